"""CPU: the training path of the attention core (include/tf_fused.h: TRAINING THROUGH THE ATTENTION CORE; trackformer_amd/csrc/mha_bwd.h
and the TRAIN instantiation of mha_core.hip's default kernel) on the emulated library -- the kernels' own source under the SIMT emulator
-- against the float64 yardsticks and the numpy restatement of the mask contract of tests/util_attention_train.py, plus the host logic
of fused.set_attention_training that needs no GPU.

Every operand lives in a buffer with NaN in the gaps between its rows; every output in one with a canary in the gaps and in three rows
behind the last, checked unchanged: a store outside the tensor fails the test."""
import numpy as np
import pytest
import torch

from tests import emu_lib
from tests import util_attention_train as AT
from tests import util_norm_attn_numerics as NA

emu = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ for the emulated library")

CANARY = np.float32(-4321.5)
SEED, OFFSET = 0x9E3779B97F4A7C15 - 2 ** 64, 0x7FEDCBA987654321
CASES = [(1, 1, 16, 16, 32), (2, 2, 37, 50, 32), (1, 2, 50, 37, 36), (1, 1, 17, 70, 32)]
MASKED = {(1, 1, 17, 70, 32)}          # the cases that run with a key mask
PROFILES = ["unit", "peaked", "qoffset"]
PS = [None, 0.1, 0.5]


def _lib():
    return emu_lib.lib()   # bound from the headers (trackformer_amd._cabi.bind)


def _rng(seed=SEED, offset=OFFSET):
    return np.array([seed, offset], dtype=np.int64)


def _in(t, ld):
    """[N, L, H, D] tensor -> aligned [N L, ld] buffer, NaN in the gaps."""
    a = t.numpy() if torch.is_tensor(t) else t
    N, L, H, D = a.shape
    return emu_lib._strided(np.ascontiguousarray(a, np.float32).reshape(N, L, H * D), ld)


def _out(N, L, E, ld):
    return emu_lib._strided(np.full((N, L, E), np.nan, np.float32), ld, CANARY, guard_rows=3)


def _take(buf, N, L, H, D, what):
    E = H * D
    assert (buf[:N * L, E:] == CANARY).all() and (buf[N * L:] == CANARY).all(), what + " wrote outside its rows"
    return torch.from_numpy(buf[:N * L, :E].reshape(N, L, H, D).copy())


def train_forward(q, k, v, scale, key_mask=None, p=None, rng=None, pad=8):
    """-> (out [N, Lq, H, D], stats [N, H, Lq, 2]) of tf_mha_core_train_f32; rows `pad` floats longer than the tensors'."""
    N, Lq, H, D = q.shape
    Lk, E = k.shape[1], H * D
    ld = E + pad
    qb, kb, vb, ob = _in(q, ld), _in(k, ld), _in(v, ld), _out(N, Lq, E, ld)
    stats = np.full((N * H * Lq + 3, 2), CANARY, np.float32)
    km = None if key_mask is None else np.ascontiguousarray(key_mask.numpy(), dtype=np.uint8)
    rc = _lib().tf_mha_core_train_f32(qb.ctypes.data, kb.ctypes.data, vb.ctypes.data, ob.ctypes.data, emu_lib._p(km), stats.ctypes.data,
                                      emu_lib._p(rng), 0.0 if p is None else p, N, Lq, Lk, H, D, ld, ld, ld, ld, scale, None)
    assert rc == 0, rc
    assert (stats[N * H * Lq:] == CANARY).all(), "stats written behind the last row"
    return _take(ob, N, Lq, H, D, "tf_mha_core_train_f32"), stats[:N * H * Lq].reshape(N, H, Lq, 2).copy()


def backward(dout, q, k, v, out, stats, scale, key_mask=None, p=None, rng=None, pad=8, packed=False):
    """-> (dq, dk, dv) of tf_mha_core_bwd_f32.  packed: dq | dk side by side in ONE [N, L, 2 E] buffer with ld = 2 E (Lq == Lk)."""
    N, Lq, H, D = q.shape
    Lk, E = k.shape[1], H * D
    ld = E + pad
    bufs = [_in(t, ld) for t in (dout, q, k, v, out)]
    st = np.ascontiguousarray(stats, np.float32)
    km = None if key_mask is None else np.ascontiguousarray(key_mask.numpy(), dtype=np.uint8)
    dvb = _out(N, Lk, E, ld)
    if packed:
        assert Lq == Lk
        qkb = _out(N, Lq, 2 * E, 2 * E)
        dq_p, dk_p, lddq, lddk = qkb.ctypes.data, qkb.ctypes.data + 4 * E, 2 * E, 2 * E
    else:
        dqb, dkb = _out(N, Lq, E, ld), _out(N, Lk, E, ld)
        dq_p, dk_p, lddq, lddk = dqb.ctypes.data, dkb.ctypes.data, ld, ld
    rc = _lib().tf_mha_core_bwd_f32(*(b.ctypes.data for b in bufs), st.ctypes.data, emu_lib._p(km), emu_lib._p(rng), 0.0 if p is None else p,
                                    dq_p, dk_p, dvb.ctypes.data, N, Lq, Lk, H, D, ld, ld, ld, ld, ld, lddq, lddk, ld, scale, None)
    assert rc == 0, rc
    dv = _take(dvb, N, Lk, H, D, "tf_mha_core_bwd_f32 (dv)")
    if packed:
        assert (qkb[N * Lq:] == CANARY).all(), "tf_mha_core_bwd_f32 wrote behind the packed gradient"
        both = torch.from_numpy(qkb[:N * Lq].reshape(N, Lq, 2, H, D).copy())
        return both[:, :, 0].contiguous(), both[:, :, 1].contiguous(), dv
    return _take(dqb, N, Lq, H, D, "tf_mha_core_bwd_f32 (dq)"), _take(dkb, N, Lk, H, D, "tf_mha_core_bwd_f32 (dk)"), dv


def run_case(case, profile, p, seed=3, dead_image=False):
    """One kernel-level case -> (got, ref, fp32, key_mask, operands)."""
    N, H, Lq, Lk, D = case
    if dead_image:
        N = 2
    q, k, v, scale = NA.attention_operands(profile, N, Lq, Lk, H, D, seed)
    dout = AT.grad_operand(N, Lq, H, D, seed)
    km = AT.masks(N, Lk, seed, last_image_dead=dead_image) if (case in MASKED or dead_image) else None
    rng = _rng() if p is not None else None
    keep = torch.from_numpy(AT.keep_mask(SEED, OFFSET, p, N, H, Lq, Lk)) if p is not None else None
    out, stats = train_forward(q, k, v, scale, km, p, rng)
    dq, dk, dv = backward(dout, q, k, v, out, stats, scale, km, p, rng)
    ref = AT.reference(q, k, v, dout, scale, km, keep, p)
    fp32 = AT.formulation(q, k, v, dout, scale, km, keep, p)
    return {"out": out, "dq": dq, "dk": dk, "dv": dv}, ref, fp32, km, (q, k, v, dout, scale, stats, rng)


# ---- the yardsticks themselves ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", NA.ATTN_PROFILES)
@pytest.mark.parametrize("p", PS)
def test_fp32_formulation_passes_the_yardsticks(profile, p):
    for case in CASES:
        N, H, Lq, Lk, D = case
        q, k, v, scale = NA.attention_operands(profile, N, Lq, Lk, H, D, 5)
        dout = AT.grad_operand(N, Lq, H, D, 5)
        km = AT.masks(N, Lk, 5) if case in MASKED else None
        keep = torch.from_numpy(AT.keep_mask(SEED, OFFSET, p, N, H, Lq, Lk)) if p is not None else None
        AT.check_fp32_alone(AT.reference(q, k, v, dout, scale, km, keep, p), AT.formulation(q, k, v, dout, scale, km, keep, p),
                            "%s %s p=%s" % (case, profile, p))


def test_reference_agrees_with_float64_autograd():
    """The closed-form backward of reference() is the autograd of its forward."""
    N, H, Lq, Lk, D = 2, 2, 9, 11, 32
    q, k, v, scale = NA.attention_operands("unit", N, Lq, Lk, H, D, 1)
    dout = AT.grad_operand(N, Lq, H, D, 1)
    km = AT.masks(N, Lk, 1)
    keep = torch.from_numpy(AT.keep_mask(SEED, OFFSET, 0.5, N, H, Lq, Lk))
    ref = AT.reference(q, k, v, dout, scale, km, keep, 0.5)
    auto = AT.formulation(q, k, v, dout, scale, km, keep, 0.5, dtype=torch.float64)
    for name in AT.OUTPUTS:
        assert torch.allclose(ref[name].ref, auto[name], rtol=1e-12, atol=1e-14), name


def test_the_mask_is_the_padded_stream():
    from tests import util_dropout_train as DT
    N, H, Lq, Lk = 1, 2, 3, 6      # Lk4 = 8: keys 6, 7 of every row consume positions nobody reads
    m = AT.keep_mask(SEED, OFFSET, 0.5, N, H, Lq, Lk)
    flat = DT.keep_mask(SEED, OFFSET, 0.5, N * H * Lq * 8)
    assert m.shape == (N, H, Lq, Lk) and 0 < m.sum() < m.size
    for r in range(N * H * Lq):
        assert np.array_equal(m.reshape(-1, Lk)[r], flat[8 * r: 8 * r + Lk].astype(bool))


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------
@emu
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_kernels_against_float64(case, profile, p):
    got, ref, fp32, km, _ = run_case(case, profile, p)
    AT.check(got, ref, fp32, km, "%s %s p=%s" % (case, profile, p))


@emu
@pytest.mark.parametrize("p", PS)
def test_an_image_without_keys_is_exactly_zero_and_leaks_nothing(p):
    """N = 2, every key of the second image masked: its out, dq, dk, dv are +0 bit for bit (AT.check through Ref.zero), also with NaN in
    its dout, and the first image does not change by a bit."""
    case = (1, 1, 17, 70, 32)
    got, ref, fp32, km, (q, k, v, dout, scale, stats, rng) = run_case(case, "unit", p, dead_image=True)
    AT.check(got, ref, fp32, km, "%s dead image p=%s" % (case, p))
    assert (stats[1] == 0).all()
    bad = dout.clone()
    bad[1] = float("nan")
    dq, dk, dv = backward(bad, q, k, v, got["out"], stats, scale, km, p, rng)
    for name, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        assert torch.equal(t, got[name]), name


@emu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_without_rng_out_is_the_inference_kernel(case):
    N, H, Lq, Lk, D = case
    q, k, v, scale = NA.attention_operands("unit", N, Lq, Lk, H, D, 7)
    km = AT.masks(N, Lk, 7) if case in MASKED else None
    out, stats = train_forward(q, k, v, scale, km)
    want = emu_lib.mha_core(q.numpy(), k.numpy(), v.numpy(), scale, None if km is None else km.numpy())
    assert np.array_equal(out.numpy().view(np.uint32), want.view(np.uint32))
    # stats: the base-2 maximum and the reciprocal sum rebuild the weights
    s = (q.double().permute(0, 2, 1, 3) @ k.double().permute(0, 2, 3, 1)) * scale * math_log2e()
    if km is not None:
        s = s.masked_fill((km != 0)[:, None, None, :], -float("inf"))
    assert torch.allclose(torch.from_numpy(stats[..., 0]).double(), s.amax(-1), rtol=1e-5, atol=1e-5)
    assert torch.allclose(torch.from_numpy(stats[..., 1]).double(), 1 / torch.exp2(s - s.amax(-1, keepdim=True)).sum(-1), rtol=1e-5)


def math_log2e():
    return 1.4426950408889634


@emu
def test_one_flipped_keep_decision_fails_the_out_check():
    """A test of the test: the numerics check is a mask check.  Per kept weight the reference with that ONE decision flipped is off by
    s_p P_ij |v_j| -- far outside 2^-20 S (1 + T) at the unit profile."""
    case, p = (2, 2, 37, 50, 32), 0.5
    got, ref, fp32, km, (q, k, v, dout, scale, stats, rng) = run_case(case, "unit", p)
    N, H, Lq, Lk, D = case
    keep = torch.from_numpy(AT.keep_mask(SEED, OFFSET, p, N, H, Lq, Lk))
    for idx in [(0, 0, 0, 0), (1, 1, 36, 49), (0, 1, 17, 3), (1, 0, 5, 48)]:   # first and last weight, an inner key, the last Philox group
        flipped = keep.clone()
        flipped[idx] = ~flipped[idx]
        wrong = AT.reference(q, k, v, dout, scale, km, flipped, p)
        _, w = NA.excess(got["out"], wrong["out"])
        assert w.value > NA.BOUND, (idx, w)


@emu
@pytest.mark.parametrize("p", [None, 0.1])
def test_two_calls_are_bit_identical(p):
    a = run_case((2, 2, 37, 50, 32), "peaked", p)[0]
    b = run_case((2, 2, 37, 50, 32), "peaked", p)[0]
    for name in AT.OUTPUTS:
        assert torch.equal(a[name], b[name]), name


@emu
@pytest.mark.parametrize("p", [None, 0.1])
def test_dq_and_dk_as_the_halves_of_one_tensor(p):
    N, H, L, D = 2, 2, 37, 36
    q, k, v, scale = NA.attention_operands("unit", N, L, L, H, D, 9)
    dout = AT.grad_operand(N, L, H, D, 9)
    rng = _rng() if p is not None else None
    out, stats = train_forward(q, k, v, scale, None, p, rng)
    sep = backward(dout, q, k, v, out, stats, scale, None, p, rng)
    one = backward(dout, q, k, v, out, stats, scale, None, p, rng, packed=True)
    for a, b, name in zip(sep, one, ("dq", "dk", "dv")):
        assert torch.equal(a, b), name


@emu
def test_error_codes_in_the_headers_order():
    L = _lib()
    one = 4096            # aligned, never dereferenced: validation fails first
    rng = _rng()
    dims = (1, 16, 16, 1, 32)

    def fwd(q=one, stats=one, rng_=None, p=0.0, dims=dims, ld=32):
        return L.tf_mha_core_train_f32(q, one, one, one, None, stats, rng_, p, *dims, ld, ld, ld, ld, 0.25, None)

    def bwd(dout=one, dq=one, stats=one, rng_=None, p=0.0, dims=dims, ld=32, lddq=32):
        return L.tf_mha_core_bwd_f32(dout, one, one, one, one, stats, None, rng_, p, dq, one, one, *dims, ld, ld, ld, ld, ld, lddq, ld, ld,
                                     0.25, None)

    for f in (fwd, bwd):
        assert f(stats=None, dims=(0, 16, 16, 1, 32)) == -1            # NULL before dimensions
        assert f(rng_=rng.ctypes.data, p=1.0, dims=(1, 16, 16, 1, 48)) == -2
        assert f(rng_=rng.ctypes.data, p=0.0) == -2 and f(rng_=rng.ctypes.data, p=float("nan")) == -2
        for bad in [(0, 16, 16, 1, 32), (1, 0, 16, 1, 32), (1, 16, 1025, 1, 32), (1, 1025, 16, 1, 32), (1, 16, 16, 1, 48), (1, 16, 16, 1, 64)]:
            assert f(dims=bad) == -2, bad
        assert f(ld=34) == -2 and f(ld=28) == -2
        assert f(stats=one + 4) == -2 and f(rng_=rng.ctypes.data + 4, p=0.5) == -2
    assert fwd(q=None) == -1 and fwd(q=one + 4) == -2
    assert bwd(dout=None) == -1 and bwd(dq=None) == -1 and bwd(dq=one + 8) == -2 and bwd(lddq=30) == -2


# ---- the host side ----------------------------------------------------------------------------------------------------------------------
def test_switch_follows_the_environment_and_returns_the_previous_setting(monkeypatch):
    from trackformer_amd import fused
    monkeypatch.delenv("TF_ATTENTION_TRAIN", raising=False)
    prev = fused.set_attention_training(None)
    try:
        assert fused.attention_training_enabled() is False
        monkeypatch.setenv("TF_ATTENTION_TRAIN", "1")
        assert fused.attention_training_enabled() is True
        assert fused.set_attention_training(False) is True and fused.attention_training_enabled() is False
        assert fused.set_attention_training(None) is False and fused.attention_training_enabled() is True
        assert set(fused.attention_train_counts()) == {"own", "own_dropout", "reference", "torch"}
    finally:
        fused.set_attention_training(prev if prev else None)


def test_with_the_switch_on_host_tensors_keep_todays_bits_and_count_torch():
    from trackformer_amd import fused
    from trackformer_amd.deformable_transformer import DeformableTransformerDecoderLayer
    torch.manual_seed(0)
    layer = DeformableTransformerDecoderLayer(d_model=64, d_ffn=32, dropout=0.0, n_levels=1, n_heads=8, n_points=1)
    tgt, pos = torch.randn(2, 5, 64, requires_grad=True), torch.randn(2, 5, 64)
    mask = torch.zeros(2, 5, dtype=torch.bool)
    mask[1, 3:] = True

    def site(t):   # the self-attention site of DeformableTransformerDecoderLayer.forward, through the layer's own method
        return layer.self_attention_training(t, pos, mask)

    assert not fused.attention_training_enabled()
    want = site(tgt)
    gw = torch.autograd.grad(want.sum(), tgt)[0]
    prev = fused.set_attention_training(True)
    try:
        fused.attention_train_counts(reset=True)
        got = site(tgt)
        gg = torch.autograd.grad(got.sum(), tgt)[0]
        assert fused.attention_train_counts() == {"own": 0, "own_dropout": 0, "reference": 0, "torch": 1}
    finally:
        fused.set_attention_training(prev if prev else None)
    assert torch.equal(got, want) and torch.equal(gg, gw)
    q = k = tgt + pos
    ref = layer.self_attn(q.transpose(0, 1), k.transpose(0, 1), tgt.transpose(0, 1), key_padding_mask=mask)[0].transpose(0, 1)
    assert torch.equal(want, ref)
