"""CPU: the backward of a linear as split products (include/tf_fused.h: THE BACKWARD OF A LINEAR; trackformer_amd/csrc/linear_bwd.h)
on the emulated library -- the kernels' own source under the SIMT emulator -- against float64 with the yardstick of
tests/util_split_numerics.py, plus the host logic of fused.linear_train that needs no GPU.

The yardstick for dw[n, k] = sum_m dy[m, n] x[m, k]: dy^T [N, M] is the product's activation, x^T [K, M] its weight, the contraction
length is M; S = |dy|^T |x|; the floor is small_floor() of the SCALED operands (s dy, t x -- what the kernel splits) divided by s t,
plus the spacing of the fp32 OUTPUT itself: the result leaves the kernel unscaled, and an fp32 number is held to an absolute 2^-149
whatever the operands' scales were (a product of 4.5e-48 -- a gradient of 1e-8 times an fp32 subnormal -- is 0 in fp32; so it is in
torch's fp32 result).  Each of the at most 64 partial sums of the weight gradient is rounded to that spacing once (half of it each)
and their sum once more: OUT_FLOOR_WGRAD = 33 x 2^-149; the input gradient's epilogue rounds twice: 2 x 2^-149.  These terms matter
for outputs of order 1e-44 and for nothing else."""
import ctypes

import numpy as np
import pytest
import torch

from tests import emu_lib
from tests import util_split_numerics as U

emu = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ for the emulated library")

ACT, WEIGHT = 0, 1
TERMS = (16, 6)
OUT_FLOOR_WGRAD = 33 * 2.0 ** -149    # (module docstring)
OUT_FLOOR_DGRAD = 2 * 2.0 ** -149


def _lib():
    return emu_lib.lib()   # bound from the headers (trackformer_amd._cabi.bind)


def _al(a):
    return emu_lib._aligned(np.asarray(a, dtype=np.float32))


def _bytes(n):
    buf = np.zeros(n + 16, np.uint8)
    off = (-buf.ctypes.data) % 16
    return buf[off:off + n]


def stats(a, role, terms, colsum=False, rows=None):
    """tf_linear_grad_stats_f32 of the first `rows` rows of a -> (scale2, colsum [C] or None); scale2: [s, 1 / s] for the activation
    role, [2, C] = (t, 1 / t) per column for the weight role."""
    L = _lib()
    a = _al(a)
    M, C = (rows or a.shape[0]), a.shape[1]
    nbytes = L.tf_linear_grad_stats_workspace_bytes(M, C, role, int(colsum))
    assert nbytes > 0
    ws = _bytes(nbytes)
    ws[:] = 0xFF
    scale2 = _al(np.full(2 if role == ACT else 2 * C, np.nan))
    cs = _al(np.full(C, np.nan)) if colsum else None
    rc = L.tf_linear_grad_stats_f32(a.ctypes.data, scale2.ctypes.data, cs.ctypes.data if colsum else None, ws.ctypes.data, nbytes, M, C,
                                    role, terms, None)
    assert rc == 0, rc
    return (scale2.copy() if role == ACT else scale2.reshape(2, C).copy()), cs


def wgrad(dy, x, terms, rows=None):
    """stats of both operands + tf_linear_wgrad_split_f32 -> (dw [N, K], s, t [K])."""
    L = _lib()
    dy, x = _al(dy), _al(x)
    M, N, K = (rows or dy.shape[0]), dy.shape[1], x.shape[1]
    s2, _ = stats(dy, ACT, terms, rows=M)
    t2, _ = stats(x, WEIGHT, terms, rows=M)
    s2a, t2a = _al(np.concatenate([s2, s2])), _al(t2.reshape(-1))
    nbytes = L.tf_linear_wgrad_workspace_bytes(M, K, N)
    assert nbytes >= 0
    ws = _bytes(max(nbytes, 16))
    ws[:] = 0xFF
    dw = _al(np.full((N, K), np.nan))
    rc = L.tf_linear_wgrad_split_f32(dy.ctypes.data, x.ctypes.data, s2a.ctypes.data, t2a.ctypes.data, dw.ctypes.data, ws.ctypes.data,
                                     nbytes, M, K, N, terms, None)
    assert rc == 0, rc
    return dw, float(s2[0]), t2[0].copy()


def pack(w, terms):
    """tf_linear_pack_weight_f32 of w [N, K]."""
    L = _lib()
    w = _al(w)
    N, K = w.shape
    nbytes = L.tf_linear_packed_bytes(K, N, terms)
    assert nbytes > 0
    pk = _bytes(nbytes)
    assert L.tf_linear_pack_weight_f32(w.ctypes.data, pk.ctypes.data, K, N, terms, None) == 0
    return pk


def dgrad(dy, w, terms, scale2=None, scaled=True):
    """tf_linear_dgrad_packed_f32: dx[M, K] = dy[M, N] . w[N, K] -> (dx, s)."""
    L = _lib()
    dy = _al(dy)
    M, N = dy.shape
    K = w.shape[1]
    pk = pack(np.ascontiguousarray(np.asarray(w, dtype=np.float32).T), terms)
    if scaled and scale2 is None:
        scale2, _ = stats(dy, ACT, terms)
    s2a = _al(np.concatenate([scale2, scale2])) if scaled else None
    dx = _al(np.full((M, K), np.nan))
    rc = L.tf_linear_dgrad_packed_f32(dy.ctypes.data, s2a.ctypes.data if scaled else None, pk.ctypes.data, dx.ctypes.data, M, K, N, terms, None)
    assert rc == 0, rc
    return dx, (float(scale2[0]) if scaled else 1.0)


def operands(profile, M, N, K, seed, dy_scale):
    """Both operands are activation-like: x from the profile, dy the same scaled by dy_scale."""
    g = torch.Generator().manual_seed(seed)
    x = U.shape_activations(torch.randn(M, K, generator=g), profile, g)
    dy = U.shape_activations(torch.randn(M, N, generator=g), profile, g) * dy_scale
    return dy, x


def check_wgrad(dw, dy, x, s, t, terms, label=""):
    """The yardstick for dw (module docstring); prints torch's fp32 result's own normalised error next to it."""
    dy, x = torch.as_tensor(dy), torch.as_tensor(x)
    dw = dw if torch.is_tensor(dw) else torch.as_tensor(np.asarray(dw))
    a, w = dy.t().contiguous(), x.t().contiguous()          # activation [N, M], weight [K, M]
    ref = a.double() @ w.double().t()
    S = a.double().abs() @ w.double().abs().t()
    t = torch.as_tensor(np.asarray(t, dtype=np.float64) if not torch.is_tensor(t) else t).double().to(w.device)   # per column of x
    floor = U.small_floor((a.double() * s).float(), (w.double() * t[:, None]).float(), terms) / (s * t[None, :]) + OUT_FLOOR_WGRAD
    fp32 = a.float() @ w.float().t()
    _, own = U.excess(fp32, ref, S, floor, fp32=fp32)
    worst = U.check(dw.to(ref.device), ref, S, floor, k=a.shape[1])
    print("%s wgrad terms %d: %.3e (torch fp32: %.3e, bound %.3e)" % (label, terms, worst.value, own.fp32_err, U.bound_for(a.shape[1])))
    return worst


def check_dgrad(dx, dy, w, s, terms, label=""):
    dy, w = torch.as_tensor(dy), torch.as_tensor(w)
    dx = dx if torch.is_tensor(dx) else torch.as_tensor(np.asarray(dx))
    wt = w.t().contiguous()                                  # the product's weight [K, N]
    ref = dy.double() @ wt.double().t()
    S = dy.double().abs() @ wt.double().abs().t()
    floor = U.small_floor((dy.double() * s).float(), wt, terms) / s + OUT_FLOOR_DGRAD
    fp32 = dy.float() @ wt.float().t()
    _, own = U.excess(fp32, ref, S, floor, fp32=fp32)
    worst = U.check(dx.to(ref.device), ref, S, floor, k=dy.shape[1])
    print("%s dgrad terms %d: %.3e (torch fp32: %.3e)" % (label, terms, worst.value, own.fp32_err))
    return worst


@pytest.fixture
def msplit():
    """Forces "wgrad_msplit" for one test; restores the previous value."""
    prev = []

    def force(n):
        prev.append(_lib().tf_msda_set_option(b"wgrad_msplit", n))
    yield force
    if prev:
        _lib().tf_msda_set_option(b"wgrad_msplit", prev[0])


# (M, N, K, forced msplit or 0 = per shape)
WGRAD_CASES = [(1, 4, 32, 0), (33, 132, 36, 0), (257, 128, 256, 0), (1000, 260, 96, 0), (4100, 32, 64, 3), (4100, 32, 64, 4)]


@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("M,N,K,force", WGRAD_CASES)
def test_wgrad_against_float64(M, N, K, force, terms, msplit):
    if force:
        msplit(force)
        assert _lib().tf_linear_wgrad_workspace_bytes(M, K, N) == force * N * K * 4   # ragged chunks: 129 slices over 3 / 4
    for i, dy_scale in enumerate((1e-6, 1e3)):
        profile = U.PROFILES[(M + N + i + terms) % len(U.PROFILES)]
        dy, x = operands(profile, M, N, K, seed=M + N + K + i, dy_scale=dy_scale)
        dw, s, t = wgrad(dy.numpy(), x.numpy(), terms)
        check_wgrad(dw, dy, x, s, t, terms, "%s x %g [%d, %d, %d]" % (profile, dy_scale, M, N, K))


@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("profile", U.PROFILES)
@pytest.mark.parametrize("M,N,K", [(70, 36, 132), (1, 4, 32)])   # (one row: a column of x is ONE value, an fp32 subnormal in edge_values)
def test_wgrad_every_profile(M, N, K, profile, terms):
    for dy_scale in (1e-6, 1e3):
        dy, x = operands(profile, M, N, K, seed=11, dy_scale=dy_scale)
        dw, s, t = wgrad(dy.numpy(), x.numpy(), terms)
        check_wgrad(dw, dy, x, s, t, terms, "%s x %g" % (profile, dy_scale))


@emu
@pytest.mark.parametrize("terms", TERMS)
def test_rows_beyond_m_are_never_read(terms):
    M, N, K = 45, 36, 40
    dy, x = operands("unit", M, N, K, seed=3, dy_scale=1.0)
    want, _, _ = wgrad(dy.numpy(), x.numpy(), terms)
    guard = 40
    dyg = np.concatenate([dy.numpy(), np.full((guard, N), np.nan, np.float32)])
    xg = np.concatenate([x.numpy(), np.full((guard, K), np.nan, np.float32)])
    got, _, _ = wgrad(dyg, xg, terms, rows=M)
    assert np.isfinite(got).all() and np.array_equal(got, want)


@emu
def test_scale_equivariance_is_bitwise():
    """What a fixed-scale fp16 scheme cannot do: (2^-20 dy, 2^7 x) gives 2^-13 times the result of (dy, x), bit for bit."""
    M, N, K = 70, 128, 64
    dy, x = operands("row_spread", M, N, K, seed=5, dy_scale=1.0)
    dy, x = dy.numpy(), x.numpy()
    base, s, t = wgrad(dy, x, 16)
    moved, s2, t2 = wgrad(dy * np.float32(2.0 ** -20), x * np.float32(2.0 ** 7), 16)
    assert s2 == s * 2.0 ** 20 and np.array_equal(t2, t * np.float32(2.0 ** -7))
    assert np.array_equal(moved, base * np.float32(2.0 ** -13))
    w = (torch.randn(N, K, generator=torch.Generator().manual_seed(6)) / N ** 0.5).numpy()
    dx, _ = dgrad(dy, w, 16)
    dx2, _ = dgrad(dy * np.float32(2.0 ** -20), w, 16)
    assert np.array_equal(dx2, dx * np.float32(2.0 ** -20))


@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("M,N,K", [(300, 128, 64), (70, 256, 256)])
def test_dgrad_is_the_packed_product_of_the_scaled_gradient(M, N, K, terms):
    g = torch.Generator().manual_seed(M)
    dy = (torch.randn(M, N, generator=g) * 3e-5).numpy()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).numpy()
    scale2, _ = stats(dy, ACT, terms)
    s = np.float32(scale2[0])
    assert (s == 1.0) == (terms == 6)
    dx, _ = dgrad(dy, w, terms, scale2=scale2)
    plain, _ = dgrad(dy * s, w, terms, scaled=False)            # tf_linear_packed_f32's arithmetic: no scale pointer
    prev = emu_lib.set_terms(terms)
    try:
        packed = emu_lib.linear_packed(dy * s, np.ascontiguousarray(w.T))
    finally:
        emu_lib.set_terms(prev)
    assert np.array_equal(plain, packed)
    assert np.array_equal(dx, packed * np.float32(scale2[1]))
    check_dgrad(dx, dy, w, float(s), terms, "[%d, %d, %d]" % (M, N, K))


@emu
def test_stats_scale_and_colsum():
    M, C = 130, 36
    g = torch.Generator().manual_seed(1)
    base = (torch.rand(M, C, generator=g) - 0.5).numpy()              # |a| < 0.5
    for e in (-30, -3, 0, 9, 40):
        for top in (np.float32(2.0 ** e), np.float32(2.0 ** e * (2.0 - 2.0 ** -23))):
            a = base * np.float32(2.0 ** e)
            a[77, 5] = -top
            s2, _ = stats(a, ACT, 16)
            assert s2[0] == np.float32(2.0 ** (14 - e)) and s2[1] == np.float32(2.0 ** (e - 14)), (e, top, s2)
            assert 2.0 ** 14 <= float(s2[0]) * float(top) < 2.0 ** 15
            assert tuple(stats(a, ACT, 6)[0]) == (1.0, 1.0)           # six bf16 terms: no scaling
            t2, _ = stats(a, WEIGHT, 16)                              # per column: column 5 holds `top`, the others their own maximum
            assert t2[0, 5] == np.float32(2.0 ** (13 - e)) and t2[1, 5] == np.float32(2.0 ** (e - 13)), (e, top, t2[:, 5])
            col = np.abs(a).max(0)
            assert ((t2[0] * col >= 2.0 ** 13) & (t2[0] * col < 2.0 ** 14)).all() and np.array_equal(t2[0] * t2[1], np.ones(C, np.float32))
            assert (stats(a, WEIGHT, 6)[0] == 1.0).all()
    for bad in (0.0, np.nan, np.inf):
        a = np.zeros((M, C), np.float32) if bad == 0.0 else base.copy()
        a[3, 7] = bad
        assert tuple(stats(a, ACT, 16)[0]) == (1.0, 1.0), bad
        t2, _ = stats(a, WEIGHT, 16)
        assert t2[0, 7] == 1.0 and t2[1, 7] == 1.0, bad          # the column that holds it (or is all zero); the others keep theirs
        assert bad == 0.0 or (t2[0, :7] > 1.0).all()
    # the bias gradient: fixed order (two calls agree bit for bit), within 2^-24 M sum |a| of float64
    for rows in (M, 4100):
        a = torch.randn(rows, C, generator=g).numpy() * np.float32(1e-3)
        _, c1 = stats(a, ACT, 16, colsum=True)
        _, c2 = stats(a, ACT, 16, colsum=True)
        assert np.array_equal(c1, c2)
        err = np.abs(c1.astype(np.float64) - a.astype(np.float64).sum(0))
        assert (err <= 2.0 ** -24 * rows * np.abs(a.astype(np.float64)).sum(0)).all(), err.max()


@emu
def test_status_codes_in_order_before_any_work(msplit):
    L = _lib()
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    big = 1 << 30
    # NULL pointer -> -1 (even with bad dimensions), K % 4 -> -2 (even with a short workspace), short workspace -> -6
    assert L.tf_linear_grad_stats_f32(None, one, None, one, big, 10, 30, 0, 16, None) == -1
    assert L.tf_linear_grad_stats_f32(one, one, None, one, 0, 10, 30, 0, 16, None) == -2
    assert L.tf_linear_grad_stats_f32(one, one, None, one, 0, 10, 32, 0, 16, None) == -6
    assert L.tf_linear_grad_stats_f32(one, one, None, one, big, 10, 32, 2, 16, None) == -2      # unknown role
    assert L.tf_linear_grad_stats_workspace_bytes(10, 30, 0, 0) == -1
    msplit(3)
    assert L.tf_linear_wgrad_split_f32(one, None, one, one, one, one, big, 4100, 30, 32, 16, None) == -1
    assert L.tf_linear_wgrad_split_f32(one, one, one, one, one, one, 0, 4100, 30, 32, 16, None) == -2
    assert L.tf_linear_wgrad_split_f32(one, one, one, one, one, one, big, 4100, 64, 30, 16, None) == -2
    assert L.tf_linear_wgrad_split_f32(one, one, one, one, one, one, big, 4100, 64, 32, 3, None) == -2    # unknown terms
    assert L.tf_linear_wgrad_split_f32(one, one, one, one, one, one, 16, 4100, 64, 32, 16, None) == -6
    assert L.tf_linear_wgrad_split_f32(one, one, one, one, one, None, big, 4100, 64, 32, 16, None) == -6
    assert L.tf_linear_wgrad_workspace_bytes(4100, 30, 32) == -1
    assert L.tf_linear_dgrad_packed_f32(one, one, None, one, 10, 64, 64, 16, None) == -1
    assert L.tf_linear_dgrad_packed_f32(one, one, one, one, 10, 64, 96, 16, None) == -2        # the contraction: N % 64
    # the option round-trips; out-of-range values mean "per shape"
    assert L.tf_msda_set_option(b"wgrad_msplit", 4) == 3
    assert L.tf_msda_set_option(b"wgrad_msplit", 1000) == 4
    assert L.tf_msda_set_option(b"wgrad_msplit", 3) == 0


# ---- host logic that needs no GPU ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    from trackformer_amd import build
    build.build_all()


def test_switch_and_environment_variable_round_trip(monkeypatch):
    from trackformer_amd import fused
    monkeypatch.delenv("TF_SPLIT_LINEAR_TRAIN", raising=False)
    fused.set_split_linear_training(None)
    try:
        assert fused.split_linear_training_enabled() is False          # the default is off
        monkeypatch.setenv("TF_SPLIT_LINEAR_TRAIN", "1")
        assert fused.split_linear_training_enabled() is True
        monkeypatch.setenv("TF_SPLIT_LINEAR_TRAIN", "0")
        assert fused.split_linear_training_enabled() is False
        assert fused.set_split_linear_training(True) is False
        assert fused.split_linear_training_enabled() is True
        assert fused.set_split_linear_training(False) is True
        assert fused.split_linear_training_enabled() is False
        assert set(fused.train_route_counts()) == {"dgrad_own", "dgrad_torch", "wgrad_own", "wgrad_torch", "bias_own", "bias_torch"}
    finally:
        fused.set_split_linear_training(None)


def test_linear_train_declines_cpu_tensors():
    from trackformer_amd import fused
    x = torch.randn(5, 32, requires_grad=True)
    w = torch.randn(8, 32, requires_grad=True)
    assert fused.linear_train(x, w, torch.zeros(8)) is None
    assert fused.linear_train(x, w, None, relu=True) is None
    assert not fused.train_route(x)


def test_cpu_msdeformattn_gradients_do_not_depend_on_the_switch(built):
    from trackformer_amd import fused
    from trackformer_amd.msda import MSDeformAttn
    torch.manual_seed(0)
    attn = MSDeformAttn(d_model=32, n_levels=2, n_heads=8, n_points=2).train()
    with torch.no_grad():
        for p in attn.parameters():
            p.add_(0.05 * torch.randn_like(p))
    shapes = torch.tensor([[4, 5], [2, 3]])
    S = 26
    query, src, ref = torch.randn(2, 7, 32), torch.randn(2, S, 32), torch.rand(2, 7, 2, 2)
    grads = []
    before = fused.train_route_counts()
    for on in (False, True):
        prev = fused.set_split_linear_training(on)
        try:
            attn.zero_grad()
            q = query.clone().requires_grad_(True)
            out = attn(q, ref, src, shapes)
            out.square().sum().backward()
            grads.append([q.grad.clone()] + [p.grad.clone() for p in attn.parameters()])
        finally:
            fused.set_split_linear_training(prev)
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    assert fused.train_route_counts() == before
