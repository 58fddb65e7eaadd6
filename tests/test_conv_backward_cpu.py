"""CPU: the backward of a 3 x 3 convolution as split products (include/tf_fused.h: THE BACKWARD OF A 3 x 3 CONVOLUTION;
trackformer_amd/csrc/conv_bwd.h) on the emulated library -- the kernels' own source under the SIMT emulator -- with the helpers and the
yardstick of tests/test_linear_backward_cpu.py, plus the host logic of fused.conv_train that needs no GPU.

Both products are products of the UNFOLDED matrix U[M, 9 cin] (tap-major columns, zeros where a tap leaves the image; M = nimg hout wout):
dw = dy^T U is held to check_wgrad(dw, dy, U, s, t repeated nine times) -- contraction length M, floor from the scaled operands --, and
dx = U(dy) . w_rot^T to check_dgrad with the contraction length 9 cout.  unfold() itself is checked against the float64 autograd of
F.conv2d on the same fp32 operands in every float64 test (the two float64 results differ by summation order only: held to 2^-40 of the
sum of magnitudes), so the reference is F.conv2d's.  The shapes are the smallest that exercise each way the addressing can go wrong."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import emu_lib
from tests.test_linear_backward_cpu import ACT, TERMS, WEIGHT, _al, _bytes, _lib
from tests.test_linear_backward_cpu import check_dgrad, check_wgrad, msplit, operands, pack, stats, wgrad as linear_wgrad  # noqa: F401

emu = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ for the emulated library")

# (nimg, h, w, cin, cout, stride, forced wgrad_msplit or 0)
WGRAD_CASES = [
    (1, 1, 1, 4, 4, 1, 0),        # one pixel: only the centre tap is non-zero
    (2, 5, 7, 36, 40, 1, 0),      # odd sizes: tiles straddle taps, the image boundary lies inside a 32-row slice
    (2, 6, 9, 64, 132, 2, 0),     # stride 2, even / odd extents
    (1, 2, 2, 8, 8, 2, 0),        # stride 2, one output pixel
    (3, 9, 11, 128, 64, 1, 3),    # 10 slices in 3 chunks (4, 4, 2) ...
    (3, 9, 11, 128, 64, 1, 4),    # ... and in 4 (3, 3, 3, 1): chunks that do not divide the slices
]
# (nimg, h, w, cin, cout, stride)
DGRAD_CASES = [(1, 1, 1, 4, 64, 1), (2, 5, 7, 36, 64, 1), (1, 9, 11, 128, 128, 1)]


def out_size(n, stride):
    return (n - 1) // stride + 1


def unfold(x, stride):
    """x [nimg, hin, win, cin] -> U [nimg hout wout, 9 cin]: column (3 ky + kx) cin + ci of row (n, ho, wo) is
    x[n, ho stride + ky - 1, wo stride + kx - 1, ci], or 0 outside the image."""
    x = np.asarray(x)
    nimg, hin, win, cin = x.shape
    hout, wout = out_size(hin, stride), out_size(win, stride)
    xp = np.zeros((nimg, hin + 2, win + 2, cin), x.dtype)
    xp[:, 1:-1, 1:-1] = x
    cols = [xp[:, ky:ky + (hout - 1) * stride + 1:stride, kx:kx + (wout - 1) * stride + 1:stride] for ky in range(3) for kx in range(3)]
    return np.ascontiguousarray(np.stack(cols, axis=3).reshape(nimg * hout * wout, 9 * cin))


def rotate(w):
    """w [cout, 3, 3, cin] -> w_rot [cin, 3, 3, cout], w_rot[ci, ky, kx, co] = w[co, 2 - ky, 2 - kx, ci]."""
    return np.ascontiguousarray(np.asarray(w)[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))


def conv_operands(profile, nimg, h, w, cin, cout, stride, seed, dy_scale):
    """dy [nimg, hout, wout, cout] and x [nimg, h, w, cin], both activation-like (operands() of the linear test)."""
    hout, wout = out_size(h, stride), out_size(w, stride)
    dy, _ = operands(profile, nimg * hout * wout, cout, 4, seed, dy_scale)
    _, x = operands(profile, nimg * h * w, 4, cin, seed + 1, 1.0)
    return dy.numpy().reshape(nimg, hout, wout, cout), x.numpy().reshape(nimg, h, w, cin)


def conv_wgrad(dy, x, stride, terms, scales=None, pointers=None):
    """stats of both operands + tf_conv3x3_wgrad_split_f32 -> (dw [cout, 9 cin], s, t [cin]).  pointers: (dy address, x address) of
    copies that live elsewhere (guard-band buffers); the statistics come from the arrays given."""
    L = _lib()
    dy, x = _al(dy), _al(x)
    nimg, hin, win, cin = x.shape
    cout = dy.shape[-1]
    assert dy.shape == (nimg, out_size(hin, stride), out_size(win, stride), cout)
    if scales is None:
        s2, _ = stats(dy.reshape(-1, cout), ACT, terms)
        t2, _ = stats(x.reshape(-1, cin), WEIGHT, terms)
    else:
        s2, t2 = scales
    s2a, t2a = _al(np.concatenate([s2, s2])), _al(t2.reshape(-1))
    nbytes = L.tf_conv3x3_wgrad_workspace_bytes(nimg, hin, win, cin, cout, stride)
    assert nbytes >= 0
    ws = _bytes(max(nbytes, 16))
    ws[:] = 0xFF
    dw = _al(np.full((cout, 9 * cin), np.nan))
    pdy, px = pointers if pointers else (dy.ctypes.data, x.ctypes.data)
    rc = L.tf_conv3x3_wgrad_split_f32(pdy, px, s2a.ctypes.data, t2a.ctypes.data, dw.ctypes.data, ws.ctypes.data, nbytes, nimg, hin, win,
                                      cin, cout, stride, terms, None)
    assert rc == 0, rc
    return dw, float(s2[0]), t2[0].copy()


def conv_dgrad(dy, w, terms, scale2=None, scaled=True, ksplit=1):
    """tf_conv3x3_dgrad_packed_f32: dy [nimg, h, w, cout], w [cout, 3, 3, cin] -> (dx [nimg, h, w, cin], s)."""
    L = _lib()
    dy = _al(dy)
    nimg, h, wd, cout = dy.shape
    cin = w.shape[-1]
    pk = pack(rotate(w).reshape(cin, 9 * cout), terms)
    if scaled and scale2 is None:
        scale2, _ = stats(dy.reshape(-1, cout), ACT, terms)
    s2a = _al(np.concatenate([scale2, scale2])) if scaled else None
    dx = _al(np.full((nimg, h, wd, cin), np.nan))
    ws = _al(np.full((ksplit, dx.size), np.nan)) if ksplit > 1 else None
    rc = L.tf_conv3x3_dgrad_packed_f32(dy.ctypes.data, s2a.ctypes.data if scaled else None, pk.ctypes.data, dx.ctypes.data,
                                       ws.ctypes.data if ksplit > 1 else None, ksplit, nimg, h, wd, cin, cout, terms, None)
    assert rc == 0, rc
    return dx, (float(scale2[0]) if scaled else 1.0)


def conv2d_float64_grads(dy, x, w, stride):
    """(dx [nimg, h, w, cin], dw [cout, 9 cin]) of F.conv2d(padding 1) in float64 on the fp32 operands."""
    xt = torch.as_tensor(np.asarray(x)).double().permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.as_tensor(np.asarray(w)).double().permute(0, 3, 1, 2).requires_grad_(True)
    y = F.conv2d(xt, wt, None, stride, 1)
    gx, gw = torch.autograd.grad(y, (xt, wt), torch.as_tensor(np.asarray(dy)).double().permute(0, 3, 1, 2))
    return gx.permute(0, 2, 3, 1).contiguous(), gw.permute(0, 2, 3, 1).reshape(gw.shape[0], -1).contiguous()


def check_conv_wgrad(dw, dy, x, stride, s, t, terms, label=""):
    """check_wgrad on the unfolded matrix, whose float64 product is first held against F.conv2d's float64 dw."""
    cout, cin = dy.shape[-1], x.shape[-1]
    Um = unfold(x, stride)
    dy2 = np.asarray(dy).reshape(-1, cout)
    _, ref = conv2d_float64_grads(dy, x, np.zeros((cout, 3, 3, cin), np.float32), stride)
    mine = torch.as_tensor(dy2).double().t() @ torch.as_tensor(Um).double()
    S = torch.as_tensor(dy2).double().abs().t() @ torch.as_tensor(Um).double().abs()
    assert ((mine - ref).abs() <= 2.0 ** -40 * S).all()
    return check_wgrad(np.asarray(dw), dy2, Um, s, np.tile(np.asarray(t), 9), terms, label)


def check_conv_dgrad(dx, dy, w, s, terms, label=""):
    """check_dgrad with U(dy) as the activation and w_rot as the weight, first held against F.conv2d's float64 dx."""
    cout, cin = dy.shape[-1], w.shape[-1]
    Ud = unfold(dy, 1)
    wr = rotate(w).reshape(cin, 9 * cout)
    ref, _ = conv2d_float64_grads(dy, np.zeros(dy.shape[:3] + (cin,), np.float32), w, 1)
    mine = torch.as_tensor(Ud).double() @ torch.as_tensor(wr).double().t()
    S = torch.as_tensor(Ud).double().abs() @ torch.as_tensor(wr).double().abs().t()
    assert ((mine - ref.reshape(-1, cin)).abs() <= 2.0 ** -40 * S).all()
    return check_dgrad(np.asarray(dx).reshape(-1, cin), Ud, np.ascontiguousarray(wr.T), s, terms, label)


def conv_weight(cout, cin, seed):
    return (torch.randn(cout, 3, 3, cin, generator=torch.Generator().manual_seed(seed)) / (9 * cin) ** 0.5).numpy()


@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout,stride,force", WGRAD_CASES)
def test_wgrad_against_float64(nimg, h, w, cin, cout, stride, force, terms, msplit):
    from tests import util_split_numerics as U
    if force:
        msplit(force)
        assert _lib().tf_conv3x3_wgrad_workspace_bytes(nimg, h, w, cin, cout, stride) == force * cout * 9 * cin * 4
    for i, dy_scale in enumerate((1e-6, 1e3)):
        profile = U.PROFILES[(h + cout + i + terms) % len(U.PROFILES)]
        dy, x = conv_operands(profile, nimg, h, w, cin, cout, stride, seed=h + w + cin + i, dy_scale=dy_scale)
        dw, s, t = conv_wgrad(dy, x, stride, terms)
        check_conv_wgrad(dw, dy, x, stride, s, t, terms, "%s x %g %s" % (profile, dy_scale, (nimg, h, w, cin, cout, stride)))
        if h == 1 and w == 1:   # one pixel: eight taps see nothing but padding
            taps = dw.reshape(cout, 9, cin)
            assert (np.delete(taps, 4, axis=1) == 0.0).all() and (taps[:, 4] != 0.0).any()


@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout,stride,force", WGRAD_CASES[1:3])
def test_wgrad_is_the_linear_wgrad_of_the_unfolded_matrix(nimg, h, w, cin, cout, stride, force, terms):
    """The same products, the same order, the same chunks: only the addressing is new."""
    L = _lib()
    dy, x = conv_operands("row_spread", nimg, h, w, cin, cout, stride, seed=7, dy_scale=3e-4)
    dw, s, t = conv_wgrad(dy, x, stride, terms)
    Um, dy2 = _al(unfold(x, stride)), _al(dy.reshape(-1, cout))
    M, K = Um.shape
    s2, _ = stats(dy2, ACT, terms)
    t2, _ = stats(x.reshape(-1, cin), WEIGHT, terms)
    s2a, t9 = _al(np.concatenate([s2, s2])), _al(np.concatenate([np.tile(t2[0], 9), np.tile(t2[1], 9)]))
    nbytes = L.tf_linear_wgrad_workspace_bytes(M, K, cout)
    assert nbytes == L.tf_conv3x3_wgrad_workspace_bytes(nimg, h, w, cin, cout, stride)
    ws = _bytes(max(nbytes, 16))
    want = _al(np.full((cout, K), np.nan))
    assert L.tf_linear_wgrad_split_f32(dy2.ctypes.data, Um.ctypes.data, s2a.ctypes.data, t9.ctypes.data, want.ctypes.data, ws.ctypes.data,
                                       nbytes, M, K, cout, terms, None) == 0
    assert np.isfinite(want).all() and np.array_equal(dw, want)


@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("stride", [1, 2])
def test_rows_and_pixels_outside_are_never_read(stride, terms):
    """NaN guard bands through offset views: the whole batch from a buffer with bands at both ends (reads in front of the first and
    behind the last image), and every image on its own (nimg = 1) from a buffer with a band between the images (reads past one image's
    end).  A read across the boundary INSIDE the batched call would fetch finite data and is not seen here: the float64 cases and the
    comparison with the unfolded matrix see it."""
    nimg, h, w, cin, cout = 2, 5, 7, 36, 40
    dy, x = conv_operands("unit", nimg, h, w, cin, cout, stride, seed=3, dy_scale=1.0)
    scales = (stats(dy.reshape(-1, cout), ACT, terms)[0], stats(x.reshape(-1, cin), WEIGHT, terms)[0])
    want, _, _ = conv_wgrad(dy, x, stride, terms, scales=scales)
    guard = 512   # floats: more than a row of the image and a multiple of four (the views stay 16-byte aligned)

    def banded(a, per_image):
        parts = [a[i:i + 1].reshape(-1) for i in range(nimg)] if per_image else [a.reshape(-1)]
        buf = _al(np.full(guard + sum(p.size + guard for p in parts), np.nan, np.float32))
        offs, o = [], guard
        for p in parts:
            buf[o:o + p.size] = p
            offs.append(buf.ctypes.data + 4 * o)
            o += p.size + guard
        return buf, offs

    bdy, ody = banded(dy, False)
    bx, ox = banded(x, False)
    got, _, _ = conv_wgrad(dy, x, stride, terms, scales=scales, pointers=(ody[0], ox[0]))
    assert np.isfinite(got).all() and np.array_equal(got, want)
    bdy, ody = banded(dy, True)
    bx, ox = banded(x, True)
    for i in range(nimg):
        one, _, _ = conv_wgrad(dy[i:i + 1], x[i:i + 1], stride, terms, scales=scales)
        got, _, _ = conv_wgrad(dy[i:i + 1], x[i:i + 1], stride, terms, scales=scales, pointers=(ody[i], ox[i]))
        assert np.isfinite(got).all() and np.array_equal(got, one)


@emu
@pytest.mark.parametrize("halo", [1, 0])
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout,stride,ksplit", [c + (1,) for c in DGRAD_CASES] + [DGRAD_CASES[2] + (3,)])
def test_dgrad_against_float64_and_the_packed_convolution(nimg, h, w, cin, cout, stride, ksplit, terms, halo):
    """Bit for bit (1 / s) . tf_conv_packed_f32(s dy, w_rot packed, the same ksplit), under either form of that entry point; and inside
    the bound.  (ksplit = 3 over 36 slices / 4 channel slices: pieces of 12 + 12 + 12 / 2 + 2.)"""
    g = torch.Generator().manual_seed(h * w + cin)
    dy = (torch.randn(nimg, h, w, cout, generator=g) * 3e-5).numpy()
    wt = conv_weight(cout, cin, seed=cin + cout)
    scale2, _ = stats(dy.reshape(-1, cout), ACT, terms)
    s = np.float32(scale2[0])
    assert (s == 1.0) == (terms == 6)
    prev = emu_lib.set_options(conv_halo=halo)
    prev_terms = emu_lib.set_terms(terms)
    try:
        dx, _ = conv_dgrad(dy, wt, terms, scale2=scale2, ksplit=ksplit)
        plain, _ = conv_dgrad(dy * s, wt, terms, scaled=False, ksplit=ksplit)
        packed = emu_lib.conv_packed(dy * s, rotate(wt), ksplit=ksplit)
    finally:
        emu_lib.set_terms(prev_terms)
        emu_lib.set_options(**prev)
    assert np.array_equal(plain, packed)
    assert np.array_equal(dx, packed * np.float32(scale2[1]))
    check_conv_dgrad(dx, dy, wt, float(s), terms, str((nimg, h, w, cin, cout)))


def linear_dgrad_splitk(dy, w, terms, ksplit):
    """tf_linear_dgrad_splitk_packed_f32: dx[M, K] = dy[M, N] . w[N, K] with the contraction over N in ksplit pieces -> (dx, s)."""
    L = _lib()
    dy = _al(dy)
    M, N = dy.shape
    K = w.shape[1]
    pk = pack(np.ascontiguousarray(np.asarray(w, dtype=np.float32).T), terms)
    scale2, _ = stats(dy, ACT, terms)
    s2a = _al(np.concatenate([scale2, scale2]))
    dx = _al(np.full((M, K), np.nan))
    ws = _al(np.full((ksplit, M * K), np.nan)) if ksplit > 1 else None
    rc = L.tf_linear_dgrad_splitk_packed_f32(dy.ctypes.data, s2a.ctypes.data, pk.ctypes.data, dx.ctypes.data,
                                             ws.ctypes.data if ksplit > 1 else None, ksplit, M, K, N, terms, None)
    assert rc == 0, rc
    return dx, float(scale2[0])


@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("M,N,K,ksplit", [(70, 256, 64, 3), (300, 128, 36, 2), (33, 1024, 128, 4)])
def test_linear_dgrad_splitk_against_float64_and_the_unsplit_entry(M, N, K, ksplit, terms):
    """The input gradient of the 1 x 1 layers: with one piece the bits of tf_linear_dgrad_packed_f32, with several inside the same
    bound (pieces of 4 + 4, 2 + 2 and 8 + 8 + 8 + 8 slices of 32)."""
    from tests.test_linear_backward_cpu import dgrad as linear_dgrad
    g = torch.Generator().manual_seed(M + N)
    dy = (torch.randn(M, N, generator=g) * 3e-5).numpy()
    w = (torch.randn(N, K, generator=g) / N ** 0.5).numpy()
    one, s = linear_dgrad_splitk(dy, w, terms, 1)
    want, _ = linear_dgrad(dy, w, terms)
    assert np.array_equal(one, want)
    dx, s = linear_dgrad_splitk(dy, w, terms, ksplit)
    assert np.isfinite(dx).all()
    check_dgrad(dx, dy, w, s, terms, "[%d, %d, %d] in %d pieces" % (M, N, K, ksplit))


@emu
def test_scale_equivariance_is_bitwise():
    """(2^-20 dy, 2^7 x) gives 2^-13 times dw, 2^-20 dy gives 2^-20 times dx, bit for bit."""
    nimg, h, w, cin, cout = 2, 5, 7, 36, 64
    dy, x = conv_operands("row_spread", nimg, h, w, cin, cout, 1, seed=5, dy_scale=1.0)
    base, s, t = conv_wgrad(dy, x, 1, 16)
    moved, s2, t2 = conv_wgrad(dy * np.float32(2.0 ** -20), x * np.float32(2.0 ** 7), 1, 16)
    assert s2 == s * 2.0 ** 20 and np.array_equal(t2, t * np.float32(2.0 ** -7))
    assert np.array_equal(moved, base * np.float32(2.0 ** -13))
    wt = conv_weight(cout, cin, seed=6)
    dx, _ = conv_dgrad(dy, wt, 16)
    dx2, _ = conv_dgrad(dy * np.float32(2.0 ** -20), wt, 16)
    assert np.array_equal(dx2, dx * np.float32(2.0 ** -20))


@emu
def test_status_codes_in_order_before_any_work(msplit):
    L = _lib()
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    odd = ctypes.c_void_p(20)
    big = 1 << 30
    msplit(3)
    wg = L.tf_conv3x3_wgrad_split_f32
    # NULL pointer -> -1 (even with bad dimensions), dimensions / alignment -> -2 (even with a short workspace), short workspace -> -6
    assert wg(one, None, one, one, one, one, big, 3, 9, 11, 30, 64, 1, 16, None) == -1
    assert wg(one, one, one, one, None, one, 0, 3, 9, 11, 30, 64, 3, 16, None) == -1
    assert wg(one, one, one, one, one, one, 0, 3, 9, 11, 30, 64, 1, 16, None) == -2      # cin % 4
    assert wg(one, one, one, one, one, one, 0, 3, 9, 11, 32, 62, 1, 16, None) == -2      # cout % 4
    assert wg(one, one, one, one, one, one, 0, 3, 9, 11, 32, 64, 3, 16, None) == -2      # stride
    assert wg(one, one, one, one, one, one, 0, 3, 9, 11, 32, 64, 1, 3, None) == -2       # unknown terms
    assert wg(one, odd, one, one, one, one, 0, 3, 9, 11, 32, 64, 1, 16, None) == -2      # alignment
    assert wg(one, one, one, one, one, one, 0, 1 << 15, 1 << 8, 1 << 8, 32, 64, 1, 16, None) == -2   # x of 256 GiB
    assert wg(one, one, one, one, one, one, 16, 3, 9, 11, 32, 64, 1, 16, None) == -6
    assert wg(one, one, one, one, one, None, big, 3, 9, 11, 32, 64, 1, 16, None) == -6
    assert wg(one, one, one, one, one, odd, big, 3, 9, 11, 32, 64, 1, 16, None) == -6
    assert L.tf_conv3x3_wgrad_workspace_bytes(3, 9, 11, 30, 64, 1) == -1
    assert L.tf_conv3x3_wgrad_workspace_bytes(3, 9, 11, 32, 64, 0) == -1
    assert L.tf_conv3x3_wgrad_workspace_bytes(3, 9, 11, 32, 64, 2) == 3 * 64 * 9 * 32 * 4
    lg = L.tf_linear_dgrad_splitk_packed_f32
    assert lg(one, one, None, one, None, 1, 10, 64, 96, 16, None) == -1
    assert lg(one, None, one, one, None, 2, 10, 62, 64, 16, None) == -1     # pieces without a workspace
    assert lg(one, None, one, one, None, 1, 10, 64, 96, 16, None) == -2     # the contraction: N % 64
    assert lg(one, None, one, one, one, 65, 10, 64, 64, 16, None) == -2
    assert lg(one, None, one, one, one, 2, 10, 62, 64, 16, None) == -2      # K % 4 with pieces
    assert lg(one, None, one, one, odd, 2, 10, 64, 64, 16, None) == -2
    dg = L.tf_conv3x3_dgrad_packed_f32
    assert dg(one, one, None, one, None, 1, 1, 9, 11, 30, 96, 16, None) == -1
    assert dg(None, None, one, one, None, 1, 1, 9, 11, 32, 64, 16, None) == -1
    assert dg(one, None, one, one, None, 2, 1, 9, 11, 30, 64, 16, None) == -1  # pieces without a workspace
    assert dg(one, None, one, one, None, 1, 1, 9, 11, 32, 96, 16, None) == -2  # the contraction: cout % 64
    assert dg(one, None, one, one, None, 1, 1, 9, 11, 30, 64, 16, None) == -2  # cin % 4
    assert dg(one, None, one, one, None, 1, 1, 9, 11, 32, 64, 5, None) == -2
    assert dg(odd, None, one, one, None, 1, 1, 9, 11, 32, 64, 16, None) == -2
    assert dg(one, None, one, one, one, 65, 1, 9, 11, 32, 64, 16, None) == -2
    assert dg(one, None, one, one, odd, 2, 1, 9, 11, 32, 64, 16, None) == -2


# ---- host logic that needs no GPU ----------------------------------------------------------------------------------------------------
def test_switch_and_environment_variable_round_trip(monkeypatch):
    from trackformer_amd import backbone, fused
    monkeypatch.delenv("TF_SPLIT_CONV_TRAIN", raising=False)
    backbone.set_split_conv_training(None)
    try:
        assert backbone.split_conv_training_enabled() is False          # the default is off
        monkeypatch.setenv("TF_SPLIT_CONV_TRAIN", "1")
        assert backbone.split_conv_training_enabled() is True
        monkeypatch.setenv("TF_SPLIT_CONV_TRAIN", "0")
        assert backbone.split_conv_training_enabled() is False
        assert backbone.set_split_conv_training(True) is False
        assert backbone.split_conv_training_enabled() is True
        assert backbone.set_split_conv_training(False) is True
        assert backbone.split_conv_training_enabled() is False
        assert backbone.set_split_conv_training(None) is False
        monkeypatch.setenv("TF_SPLIT_CONV_TRAIN", "1")
        assert backbone.split_conv_training_enabled() is True           # None follows the environment again
        assert set(fused.conv_train_counts()) == {"fwd_own", "fwd_torch", "dgrad_own", "dgrad_torch", "wgrad_own", "wgrad_torch"}
    finally:
        backbone.set_split_conv_training(None)


def test_conv_train_declines_cpu_tensors():
    from trackformer_amd import fused
    before = fused.conv_train_counts()
    x = torch.randn(1, 8, 5, 6, requires_grad=True).contiguous(memory_format=torch.channels_last)
    w3 = torch.randn(64, 72, requires_grad=True)
    w1 = torch.randn(64, 8, requires_grad=True)
    assert fused.conv_train(x, w3, 1) is None
    assert fused.conv_train(x, w3, 2) is None
    assert fused.conv_train(x, w1, 1) is None
    assert fused.conv_train_counts() == before
