"""CPU: the backward of the stride-2 convolutions as split products (include/tf_fused.h: THE BACKWARD OF THE STRIDE-2 CONVOLUTIONS;
trackformer_amd/csrc/conv_strided_bwd.h) on the emulated library -- the kernels' own source under the SIMT emulator -- with the helpers
and the yardsticks of tests/test_linear_backward_cpu.py and tests/test_conv_backward_cpu.py, plus the host logic of the new branch of
fused.conv_train that needs no GPU.

The input gradient of y = conv(x, w, stride 2) splits by the parity (py, px) of the input pixel into four stride-1 products over dy:
class (py, px) is U_c(dy) [pixels of the class, T_c cout] . W_c^T with T_c = (1 + py)(1 + px) taps.  Every class is held to check_dgrad
on ITS OWN unfolded matrix and weight -- contraction length T_c cout, so the one-tap class is held to a bound four times tighter than
the four-tap class and no zero tap loosens anything.  The float64 product assembled from the four classes is first held to the
float64 autograd of F.conv2d on the same fp32 operands (2^-40 of the sum of magnitudes: summation order only), so the reference is
F.conv2d's.  The weight gradient of the strided 1 x 1 is the product of dy with the gathered matrix G = x[:, ::2, ::2]: check_wgrad
on G, and the bits of tf_linear_wgrad_split_f32 on G."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import emu_lib
from tests.test_conv_backward_cpu import conv2d_float64_grads, conv_operands, conv_weight, out_size
from tests.test_linear_backward_cpu import ACT, TERMS, WEIGHT, _al, _bytes, _lib, check_dgrad, check_wgrad, pack, stats
from tests.test_linear_backward_cpu import msplit  # noqa: F401  (fixture)

emu = pytest.mark.skipif(not emu_lib.available(), reason="no host clang++ for the emulated library")

# (nimg, h, w, cin, cout, ksplit): the input gradient of the stride-2 3 x 3
DGRAD3_CASES = [
    (1, 1, 1, 4, 64, 1),        # one pixel: one class, one tap
    (1, 2, 2, 8, 64, 1),        # every class holds one pixel, every + 1 neighbour is outside
    (2, 5, 7, 36, 64, 1),       # odd extents: four class sizes, an image boundary inside a row block
    (2, 6, 9, 64, 128, 1),      # even and odd extents
    (1, 17, 33, 8, 64, 1),      # class (0, 0) has 153 rows: more than one row block
    (1, 9, 11, 128, 128, 1),
    (1, 9, 11, 128, 128, 3),    # pieces of 6 + 6 + 4 slices (four taps), 4 + 4 (two taps), one piece (one tap)
]
# (nimg, h, w, cin, cout): the input gradient of the strided 1 x 1
DGRAD1_CASES = [(1, 2, 2, 8, 64), (2, 5, 7, 36, 64), (2, 6, 9, 64, 128)]
# (nimg, h, w, cin, cout, forced wgrad_msplit or 0): the weight gradient of the strided 1 x 1
WGRAD1_CASES = [
    (1, 1, 1, 4, 4, 0),
    (2, 5, 7, 36, 40, 0),
    (2, 6, 9, 64, 132, 0),
    (3, 17, 21, 64, 64, 3),     # 297 gathered rows = 10 slices in 3 chunks (4, 4, 2) ...
    (3, 17, 21, 64, 64, 4),     # ... and in 4 (3, 3, 3, 1): chunks that do not divide the slices
]

TAPS = ((1,), (2, 0))   # by parity: the tap rows (columns) in the order of the dy rows (columns) a, a + 1 they read
CLASSES = [(py, px) for py in (0, 1) for px in (0, 1)]


def class_size(n, parity):
    return (n - parity + 1) // 2


def class_weights(w, ks):
    """w [cout, 3, 3, cin] (or [cout, cin] for ks = 1) -> the class weights W_c [cin, T_c cout], column t cout + co = w[co, ky, kx, ci]."""
    w = np.asarray(w)
    if ks == 1:
        return [np.ascontiguousarray(w.T)]
    cin = w.shape[-1]
    return [np.ascontiguousarray(np.stack([w[:, ky, kx] for ky in TAPS[py] for kx in TAPS[px]]).transpose(2, 0, 1).reshape(cin, -1))
            for py, px in CLASSES]


def class_unfold(dy, h, w, py, px, ks=3):
    """U_c(dy) [nimg hc wc, T_c cout]: the window (a + da, b + db) of the class pixel (a, b), zeros where a + 1 = ho / b + 1 = wo."""
    dy = np.asarray(dy)
    nimg, ho, wo, cout = dy.shape
    hc, wc = class_size(h, py), class_size(w, px)
    pad = np.zeros((nimg, ho + 1, wo + 1, cout), dy.dtype)
    pad[:, :ho, :wo] = dy
    ty, tx = (1 + py, 1 + px) if ks == 3 else (1, 1)
    cols = [pad[:, da:da + hc, db:db + wc] for da in range(ty) for db in range(tx)]
    return np.ascontiguousarray(np.stack(cols, axis=3).reshape(nimg * hc * wc, -1))


def pack_classes(w, ks, terms):
    """The class images one behind the other (the `wcls_packed` of tf_conv_dgrad_stride2_packed_f32)."""
    parts = [pack(wc, terms) for wc in class_weights(w, ks)]
    buf = _bytes(sum(p.size for p in parts))
    o = 0
    for p in parts:
        buf[o:o + p.size] = p
        o += p.size
    return buf


def strided_dgrad(dy, w, h, wd, ks, terms, scale2=None, scaled=True, ksplit=1, pointers=None):
    """tf_conv_dgrad_stride2_packed_f32: dy [nimg, ho, wo, cout] -> (dx [nimg, h, wd, cin] from a NaN-filled buffer, s).  pointers:
    (dy address, packed address, dx address) of buffers that live elsewhere (guard bands); dx is then not returned."""
    L = _lib()
    dy = _al(dy)
    nimg, ho, wo, cout = dy.shape
    assert (ho, wo) == (out_size(h, 2), out_size(wd, 2))
    cin = np.asarray(w).shape[-1]
    pk = pack_classes(w, ks, terms)
    if scaled and scale2 is None:
        scale2, _ = stats(dy.reshape(-1, cout), ACT, terms)
    s2a = _al(np.concatenate([scale2, scale2])) if scaled else None
    dx = _al(np.full((nimg, h, wd, cin), np.nan))
    nbytes = L.tf_conv_dgrad_stride2_workspace_bytes(nimg, h, wd, cin, cout, ks, ksplit)
    assert nbytes > 0
    ws = _bytes(nbytes)
    ws[:] = 0xFF   # (NaN as floats)
    pdy, ppk, pdx = pointers if pointers else (dy.ctypes.data, pk.ctypes.data, dx.ctypes.data)
    rc = L.tf_conv_dgrad_stride2_packed_f32(pdy, s2a.ctypes.data if scaled else None, ppk, pdx, ws.ctypes.data, nbytes, ksplit, nimg, h, wd,
                                            cin, cout, ks, terms, None)
    assert rc == 0, rc
    return dx, (float(scale2[0]) if scaled else 1.0)


def conv1x1_float64_dx(dy, w, h, wd):
    """dx [nimg, h, wd, cin] of F.conv2d(x, w [cout, cin, 1, 1], stride 2, no padding) in float64 on the fp32 operands."""
    dy, w = np.asarray(dy), np.asarray(w)
    xt = torch.zeros(dy.shape[0], w.shape[1], h, wd, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xt, torch.as_tensor(w).double()[:, :, None, None], None, 2, 0)
    (gx,) = torch.autograd.grad(y, xt, torch.as_tensor(dy).double().permute(0, 3, 1, 2))
    return gx.permute(0, 2, 3, 1).contiguous()


def check_strided_dgrad(dx, dy, w, s, terms, ks=3, label=""):
    """Every parity class against check_dgrad on its own unfolded matrix (contraction length T_c cout); the float64 product assembled
    from the classes first held against F.conv2d's float64 dx.  ks = 1: class (0, 0) alone, the other pixels must be +0.0 bit for
    bit.  -> the worst normalised excess over the classes."""
    dx, dy = np.asarray(dx), np.asarray(dy)
    nimg, h, wd, cin = dx.shape
    assert not np.isnan(dx).any(), "an element of dx was never written"
    if ks == 3:
        ref = conv2d_float64_grads(dy, np.zeros((nimg, h, wd, cin), np.float32), w, 2)[0]
    else:
        ref = conv1x1_float64_dx(dy, w, h, wd)
    mine, S = torch.zeros_like(ref), torch.zeros_like(ref)
    worst = None
    for (py, px), wc in zip(CLASSES, class_weights(w, ks)):
        rows = dx[:, py::2, px::2]
        if rows.size == 0:
            continue
        Uc = class_unfold(dy, h, wd, py, px, ks)
        prod = torch.as_tensor(Uc).double() @ torch.as_tensor(wc).double().t()
        mine[:, py::2, px::2] = prod.reshape(rows.shape)
        S[:, py::2, px::2] = (torch.as_tensor(Uc).double().abs() @ torch.as_tensor(wc).double().abs().t()).reshape(rows.shape)
        got = check_dgrad(rows.reshape(-1, cin), Uc, np.ascontiguousarray(wc.T), s, terms, "%s class (%d, %d)" % (label, py, px))
        worst = got if worst is None or got.value > worst.value else worst
    assert ((mine - ref).abs() <= 2.0 ** -40 * S).all()
    if ks == 1:
        rest = np.ones(dx.shape[1:3], bool)
        rest[::2, ::2] = False
        zeros = dx[:, rest]
        assert (zeros.view(np.uint32) == 0).all(), "a pixel outside class (0, 0) is not +0.0"
    return worst


def strided_wgrad(dy, x, terms, scales=None, pointers=None):
    """stats of both operands + tf_conv1x1_strided_wgrad_split_f32 (stride 2) -> (dw [cout, cin], s2, t2)."""
    L = _lib()
    dy, x = _al(dy), _al(x)
    nimg, hin, win, cin = x.shape
    cout = dy.shape[-1]
    assert dy.shape == (nimg, out_size(hin, 2), out_size(win, 2), cout)
    if scales is None:
        s2, _ = stats(dy.reshape(-1, cout), ACT, terms)
        t2, _ = stats(x.reshape(-1, cin), WEIGHT, terms)   # over ALL pixels of x, as the 3 x 3 stride-2 weight gradient takes them
    else:
        s2, t2 = scales
    s2a, t2a = _al(np.concatenate([s2, s2])), _al(t2.reshape(-1))
    nbytes = L.tf_conv1x1_strided_wgrad_workspace_bytes(nimg, hin, win, cin, cout, 2)
    assert nbytes >= 0
    ws = _bytes(max(nbytes, 16))
    ws[:] = 0xFF
    # dw between bands of a sentinel that must survive: nothing outside dw is written
    bdw, adw, wdw = banded([np.full((cout, cin), np.nan, np.float32)], 512, np.float32(-7.0))
    pdy, px = pointers if pointers else (dy.ctypes.data, x.ctypes.data)
    rc = L.tf_conv1x1_strided_wgrad_split_f32(pdy, px, s2a.ctypes.data, t2a.ctypes.data, adw[0], ws.ctypes.data, nbytes, nimg, hin, win,
                                              cin, cout, 2, terms, None)
    assert rc == 0, rc
    assert (bdw[:wdw[0].start] == np.float32(-7.0)).all() and (bdw[wdw[0].stop:] == np.float32(-7.0)).all(), "a write outside dw"
    return bdw[wdw[0]].reshape(cout, cin), s2, t2


def gathered(x):
    x = np.asarray(x)
    return np.ascontiguousarray(x[:, ::2, ::2].reshape(-1, x.shape[-1]))


def linear_wgrad_with(dy2, G, s2, t2, terms):
    """tf_linear_wgrad_split_f32 on the gathered matrix with the scales given."""
    L = _lib()
    dy2, G = _al(dy2), _al(G)
    M, K = G.shape
    N = dy2.shape[1]
    s2a, t2a = _al(np.concatenate([s2, s2])), _al(t2.reshape(-1))
    nbytes = L.tf_linear_wgrad_workspace_bytes(M, K, N)
    ws = _bytes(max(nbytes, 16))
    want = _al(np.full((N, K), np.nan))
    assert L.tf_linear_wgrad_split_f32(dy2.ctypes.data, G.ctypes.data, s2a.ctypes.data, t2a.ctypes.data, want.ctypes.data, ws.ctypes.data, nbytes,
                                       M, K, N, terms, None) == 0
    return want, nbytes


def banded(parts, guard, fill=np.nan, dtype=np.float32):
    """The arrays of `parts` in one buffer with `guard` elements of `fill` in front of, between and behind them -> (buffer, addresses,
    slices)."""
    flat = [np.ascontiguousarray(p).reshape(-1) for p in parts]
    buf = emu_lib._aligned16(np.full(guard + sum(p.size + guard for p in flat), fill, dtype))
    addr, where, o = [], [], guard
    for p in flat:
        buf[o:o + p.size] = p
        addr.append(buf.ctypes.data + buf.itemsize * o)
        where.append(slice(o, o + p.size))
        o += p.size + guard
    return buf, addr, where


# ---- the stride-2 3 x 3 input gradient ------------------------------------------------------------------------------------------------
@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout,ksplit", DGRAD3_CASES)
def test_dgrad3_against_float64_per_parity_class(nimg, h, w, cin, cout, ksplit, terms):
    from tests import util_split_numerics as U
    for i, dy_scale in enumerate((1e-6, 1e3)):
        profile = U.PROFILES[(h + cout + i + terms) % len(U.PROFILES)]
        dy, _ = conv_operands(profile, nimg, h, w, cin, cout, 2, seed=h + w + cin + i, dy_scale=dy_scale)
        wt = conv_weight(cout, cin, seed=cin + cout + i)
        dx, s = strided_dgrad(dy, wt, h, w, 3, terms, ksplit=ksplit)
        check_strided_dgrad(dx, dy, wt, s, terms, 3, "%s x %g %s" % (profile, dy_scale, (nimg, h, w, cin, cout, ksplit)))


@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("ks,nimg,h,w,cin,cout,ksplit", [(3,) + DGRAD3_CASES[2], (3,) + DGRAD3_CASES[6], (1,) + DGRAD1_CASES[2] + (2,)])
def test_dgrad_is_the_plain_product_of_the_scaled_gradient(ks, nimg, h, w, cin, cout, ksplit, terms):
    """With dy_scale2 the result is (1 / s) times the plain instantiation on s dy, bit for bit (both factors are powers of two)."""
    g = torch.Generator().manual_seed(h * w + cin)
    dy = (torch.randn(nimg, out_size(h, 2), out_size(w, 2), cout, generator=g) * 3e-5).numpy()
    wt = conv_weight(cout, cin, seed=cin + cout)
    wt = wt if ks == 3 else np.ascontiguousarray(wt[:, 1, 1])
    scale2, _ = stats(dy.reshape(-1, cout), ACT, terms)
    s = np.float32(scale2[0])
    assert (s == 1.0) == (terms == 6)
    dx, _ = strided_dgrad(dy, wt, h, w, ks, terms, scale2=scale2, ksplit=ksplit)
    plain, _ = strided_dgrad(dy * s, wt, h, w, ks, terms, scaled=False, ksplit=ksplit)
    assert np.isfinite(plain).all() and np.array_equal(dx, plain * np.float32(scale2[1]))
    again, _ = strided_dgrad(dy, wt, h, w, ks, terms, scale2=scale2, ksplit=ksplit)
    assert np.array_equal(dx, again)


@emu
def test_dgrad_pieces_change_the_order_of_the_sum_only():
    """ksplit = 1 and ksplit = 3 both inside the bound (the cases above); here: they are different sums (the pieces are real), and a
    class too short to be cut gives the same bits either way."""
    nimg, h, w, cin, cout = 1, 9, 11, 128, 128
    g = torch.Generator().manual_seed(5)
    dy = torch.randn(nimg, 5, 6, cout, generator=g).numpy()
    wt = conv_weight(cout, cin, seed=9)
    one, _ = strided_dgrad(dy, wt, h, w, 3, 16, ksplit=1)
    three, _ = strided_dgrad(dy, wt, h, w, 3, 16, ksplit=3)
    assert np.array_equal(one[:, ::2, ::2], three[:, ::2, ::2])          # one tap, 128 products: one piece whatever ksplit
    assert not np.array_equal(one[:, 1::2, 1::2], three[:, 1::2, 1::2])  # four taps in three pieces
    L = _lib()
    per = [nimg * class_size(h, py) * class_size(w, px) * cin * 4 for py, px in CLASSES]
    assert L.tf_conv_dgrad_stride2_workspace_bytes(nimg, h, w, cin, cout, 3, 1) == sum(per)
    assert L.tf_conv_dgrad_stride2_workspace_bytes(nimg, h, w, cin, cout, 3, 3) == per[0] + 2 * per[1] + 2 * per[2] + 3 * per[3]
    assert L.tf_conv_dgrad_stride2_workspace_bytes(nimg, h, w, cin, cout, 1, 3) == 2 * per[0]   # 128 products: two pairs of slices


# ---- the strided 1 x 1 ------------------------------------------------------------------------------------------------------------------
@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout", DGRAD1_CASES)
def test_dgrad1_against_float64_and_exact_zeros(nimg, h, w, cin, cout, terms):
    from tests import util_split_numerics as U
    for i, dy_scale in enumerate((1e-6, 1e3)):
        profile = U.PROFILES[(h + cout + i + terms) % len(U.PROFILES)]
        dy, _ = conv_operands(profile, nimg, h, w, cin, cout, 2, seed=h + w + cin + i, dy_scale=dy_scale)
        wt = np.ascontiguousarray(conv_weight(cout, cin, seed=cin + cout + i)[:, 1, 1]) * np.float32(3.0)
        dx, s = strided_dgrad(dy, wt, h, w, 1, terms)
        check_strided_dgrad(dx, dy, wt, s, terms, 1, "1 x 1 %s x %g %s" % (profile, dy_scale, (nimg, h, w, cin, cout)))


@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("nimg,h,w,cin,cout,force", WGRAD1_CASES)
def test_wgrad1_against_float64_and_the_linear_wgrad_of_the_gathered_matrix(nimg, h, w, cin, cout, force, terms, msplit):
    from tests import util_split_numerics as U
    L = _lib()
    if force:
        msplit(force)
        assert L.tf_conv1x1_strided_wgrad_workspace_bytes(nimg, h, w, cin, cout, 2) == force * cout * cin * 4
    for i, dy_scale in enumerate((1e-6, 1e3)):
        profile = U.PROFILES[(h + cout + i + terms) % len(U.PROFILES)]
        dy, x = conv_operands(profile, nimg, h, w, cin, cout, 2, seed=h + w + cin + i, dy_scale=dy_scale)
        dw, s2, t2 = strided_wgrad(dy, x, terms)
        assert np.isfinite(dw).all()
        G, dy2 = gathered(x), dy.reshape(-1, cout)
        check_wgrad(dw, dy2, G, float(s2[0]), t2[0], terms, "1 x 1 %s x %g %s" % (profile, dy_scale, (nimg, h, w, cin, cout)))
        want, nbytes = linear_wgrad_with(dy2, G, s2, t2, terms)
        assert nbytes == L.tf_conv1x1_strided_wgrad_workspace_bytes(nimg, h, w, cin, cout, 2)
        assert np.array_equal(dw, want)   # the same products, the same order, the same chunks: only the addressing is new


# ---- guard bands --------------------------------------------------------------------------------------------------------------------------
@emu
@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("ks", [3, 1])
def test_dgrad_reads_and_writes_nothing_outside_its_tensors(ks, terms):
    """dy and the packed class images between NaN bands (a read outside reaches dx as NaN or changes its bits), dx between bands of a
    sentinel that must survive; then every image on its own from a buffer with a band between the images (a read past one image's
    end).  The emulator's own bounds checks of the buffer resources stay on."""
    nimg, h, w, cin, cout = 2, 5, 7, 36, 64
    dy, _ = conv_operands("unit", nimg, h, w, cin, cout, 2, seed=3, dy_scale=1.0)
    wt = conv_weight(cout, cin, seed=4)
    wt = wt if ks == 3 else np.ascontiguousarray(wt[:, 1, 1])
    scale2, _ = stats(dy.reshape(-1, cout), ACT, terms)
    want, _ = strided_dgrad(dy, wt, h, w, ks, terms, scale2=scale2)
    guard = 512   # floats: more than a row of dy, a multiple of four (the views stay 16-byte aligned)
    pk = pack_classes(wt, ks, terms)
    bpk, apk, _ = banded([pk], 4 * guard, 0xFF, np.uint8)

    def run(dys, n):
        bdy, ady, _ = banded(dys, guard)
        outs = [np.full((n, h, w, cin), np.nan, np.float32) for _ in dys]
        bdx, adx, wdx = banded(outs, guard, np.float32(-7.0))
        for i, d in enumerate(dys):
            strided_dgrad(d, wt, h, w, ks, terms, scale2=scale2, pointers=(ady[i], apk[0], adx[i]))
        keep = np.ones(bdx.size, bool)
        for sl in wdx:
            keep[sl] = False
        assert (bdx[keep] == np.float32(-7.0)).all(), "a write outside dx"
        return [bdx[sl].reshape(n, h, w, cin) for sl in wdx]

    got = run([dy], nimg)[0]
    assert np.isfinite(got).all() and np.array_equal(got, want)
    for i, one in enumerate(run([dy[i:i + 1] for i in range(nimg)], 1)):
        assert np.isfinite(one).all() and np.array_equal(one[0], want[i])   # (an image's result does not depend on its neighbours)
    assert (bpk[:4 * guard] == 0xFF).all() and (bpk[-4 * guard:] == 0xFF).all()


@emu
@pytest.mark.parametrize("terms", TERMS)
def test_wgrad1_reads_nothing_outside_its_tensors(terms):
    """dy and x between NaN bands, the whole batch and every image on its own; dw lies between sentinel bands in EVERY call of
    strided_wgrad (checked there)."""
    nimg, h, w, cin, cout = 2, 5, 7, 36, 40
    dy, x = conv_operands("unit", nimg, h, w, cin, cout, 2, seed=3, dy_scale=1.0)
    scales = (stats(dy.reshape(-1, cout), ACT, terms)[0], stats(x.reshape(-1, cin), WEIGHT, terms)[0])
    want, _, _ = strided_wgrad(dy, x, terms, scales=scales)
    guard = 512
    _b1, ady, _ = banded([dy], guard)
    _b2, ax, _ = banded([x], guard)
    got, _, _ = strided_wgrad(dy, x, terms, scales=scales, pointers=(ady[0], ax[0]))
    assert np.isfinite(got).all() and np.array_equal(got, want)
    _b1, ady, _ = banded([dy[i:i + 1] for i in range(nimg)], guard)
    _b2, ax, _ = banded([x[i:i + 1] for i in range(nimg)], guard)
    for i in range(nimg):
        one, _, _ = strided_wgrad(dy[i:i + 1], x[i:i + 1], terms, scales=scales)
        got, _, _ = strided_wgrad(dy[i:i + 1], x[i:i + 1], terms, scales=scales, pointers=(ady[i], ax[i]))
        assert np.isfinite(got).all() and np.array_equal(got, one)


# ---- gates ----------------------------------------------------------------------------------------------------------------------------------
@emu
def test_status_codes_in_order_before_any_work(msplit):
    L = _lib()
    one = ctypes.c_void_p(16)   # never dereferenced: validation fails first
    odd = ctypes.c_void_p(20)
    big = 1 << 40
    dg = L.tf_conv_dgrad_stride2_packed_f32
    # (dy, dy_scale2, wcls_packed, dx, workspace, workspace_bytes, ksplit, nimg, h, w, cin, cout, ks, terms, stream)
    assert dg(None, None, one, one, one, big, 1, 1, 9, 11, 32, 64, 3, 16, None) == -1
    assert dg(one, None, None, one, one, big, 1, 1, 9, 11, 30, 96, 3, 16, None) == -1     # NULL first, even with bad dimensions
    assert dg(one, None, one, None, one, big, 1, 1, 9, 11, 32, 64, 3, 16, None) == -1
    assert dg(one, None, one, one, None, big, 1, 1, 9, 11, 32, 64, 3, 16, None) == -1
    assert dg(one, None, one, one, one, 0, 1, 1, 9, 11, 32, 96, 3, 16, None) == -2        # the contraction: cout % 64 (before the workspace)
    assert dg(one, None, one, one, one, big, 1, 1, 9, 11, 30, 64, 3, 16, None) == -2      # cin % 4
    assert dg(one, None, one, one, one, big, 1, 1, 9, 11, 32, 64, 2, 16, None) == -2      # ks
    assert dg(one, None, one, one, one, big, 1, 1, 9, 11, 32, 64, 3, 5, None) == -2       # unknown terms
    assert dg(one, None, one, one, one, big, 0, 1, 9, 11, 32, 64, 3, 16, None) == -2      # ksplit
    assert dg(one, None, one, one, one, big, 65, 1, 9, 11, 32, 64, 3, 16, None) == -2
    assert dg(one, None, one, one, one, big, 1, 0, 9, 11, 32, 64, 3, 16, None) == -2
    assert dg(one, None, one, one, one, big, 1, 1 << 15, 1 << 8, 1 << 8, 32, 64, 3, 16, None) == -2   # dx of 256 GiB
    assert dg(one, None, one, one, one, big, 1, 3, 1 << 12, 1 << 12, 4, 64, 1, 16, None) == -2        # dx of 0.75 GiB, dy of 3 GiB
    for bad in range(5):
        args = [one, None, one, one, one]
        if bad == 1:
            continue
        args[bad] = odd
        assert dg(*args, big, 1, 1, 9, 11, 32, 64, 3, 16, None) == -2                      # alignment
    assert dg(one, None, one, one, one, 16, 1, 1, 9, 11, 32, 64, 3, 16, None) == -6
    assert L.tf_conv_dgrad_stride2_workspace_bytes(1, 9, 11, 30, 64, 3, 1) == -1
    assert L.tf_conv_dgrad_stride2_workspace_bytes(1, 9, 11, 32, 96, 3, 1) == -1
    assert L.tf_conv_dgrad_stride2_workspace_bytes(1, 9, 11, 32, 64, 3, 0) == -1
    assert L.tf_conv_dgrad_stride2_workspace_bytes(1, 9, 11, 32, 64, 2, 1) == -1
    assert L.tf_conv_dgrad_stride2_workspace_bytes(1, 9, 11, 32, 64, 3, 1) == 9 * 11 * 32 * 4
    assert L.tf_conv_dgrad_stride2_workspace_bytes(1, 9, 11, 32, 64, 1, 1) == 5 * 6 * 32 * 4
    msplit(3)
    wg = L.tf_conv1x1_strided_wgrad_split_f32
    # (dy, x, dy_scale2, x_scale2, dw, workspace, workspace_bytes, nimg, hin, win, cin, cout, stride, terms, stream)
    assert wg(one, None, one, one, one, one, big, 3, 17, 21, 30, 64, 2, 16, None) == -1
    assert wg(one, one, one, one, None, one, 0, 3, 17, 21, 32, 64, 3, 16, None) == -1
    assert wg(one, one, one, one, one, one, 0, 3, 17, 21, 30, 64, 2, 16, None) == -2      # cin % 4
    assert wg(one, one, one, one, one, one, 0, 3, 17, 21, 32, 62, 2, 16, None) == -2      # cout % 4
    assert wg(one, one, one, one, one, one, 0, 3, 17, 21, 32, 64, 3, 16, None) == -2      # stride
    assert wg(one, one, one, one, one, one, big, 3, 17, 21, 32, 64, 1, 16, None) == -2    # stride 1 is the linears' weight gradient
    assert L.tf_conv1x1_strided_wgrad_workspace_bytes(3, 17, 21, 32, 64, 1) == -1
    assert wg(one, one, one, one, one, one, 0, 3, 17, 21, 32, 64, 2, 3, None) == -2       # unknown terms
    assert wg(one, odd, one, one, one, one, 0, 3, 17, 21, 32, 64, 2, 16, None) == -2      # alignment
    assert wg(one, one, one, one, one, one, 0, 1 << 15, 1 << 8, 1 << 8, 32, 64, 2, 16, None) == -2   # x of 256 GiB
    assert wg(one, one, one, one, one, one, 16, 3, 17, 21, 32, 64, 2, 16, None) == -6
    assert wg(one, one, one, one, one, None, big, 3, 17, 21, 32, 64, 2, 16, None) == -6
    assert wg(one, one, one, one, one, odd, big, 3, 17, 21, 32, 64, 2, 16, None) == -6
    assert L.tf_conv1x1_strided_wgrad_workspace_bytes(3, 17, 21, 30, 64, 2) == -1
    assert L.tf_conv1x1_strided_wgrad_workspace_bytes(3, 17, 21, 32, 64, 0) == -1
    assert L.tf_conv1x1_strided_wgrad_workspace_bytes(3, 17, 21, 32, 64, 2) == 3 * 64 * 32 * 4


# ---- host logic that needs no GPU ------------------------------------------------------------------------------------------------------------
def test_switch_and_environment_variable_round_trip(monkeypatch):
    from trackformer_amd import fused
    monkeypatch.delenv("TF_STRIDED_CONV_TRAIN", raising=False)
    fused.set_strided_conv_training(None)
    try:
        assert fused.strided_conv_training_enabled() is False          # the default is off
        monkeypatch.setenv("TF_STRIDED_CONV_TRAIN", "1")
        assert fused.strided_conv_training_enabled() is True
        monkeypatch.setenv("TF_STRIDED_CONV_TRAIN", "0")
        assert fused.strided_conv_training_enabled() is False
        epoch = fused.route_epoch()
        assert fused.set_strided_conv_training(True) is False
        assert fused.route_epoch() != epoch                            # (_switched: captured graphs of the other route are dropped)
        assert fused.strided_conv_training_enabled() is True
        assert fused.set_strided_conv_training(False) is True
        assert fused.set_strided_conv_training(None) is False
        assert set(fused.conv_train_counts()) == {"fwd_own", "fwd_torch", "dgrad_own", "dgrad_torch", "wgrad_own", "wgrad_torch"}
    finally:
        fused.set_strided_conv_training(None)


def test_gates_and_pieces_are_functions_of_the_shape():
    from trackformer_amd import fused
    assert fused._strided_dgrad_gates(2, 13, 18, 64, 128)
    assert not fused._strided_dgrad_gates(2, 13, 18, 64, 32)      # the contraction: cout % 64
    assert not fused._strided_dgrad_gates(2, 13, 18, 30, 64)      # cin % 4
    assert not fused._strided_dgrad_gates(1 << 10, 1 << 10, 1 << 10, 4, 64)   # dx of 16 GiB
    # layer3.0.conv2 and the projections of layer3 / layer4 at two small images: few workgroups under a long sum -> pieces
    policy = fused._STRIDED_DGRAD_KSPLIT_POLICY
    assert fused._strided_dgrad_ksplit(2, 16, 20, 256, 256, 3) == fused._conv_ksplit(2 * 8 * 10, 4 * 256, 256, policy) == 4
    assert fused._strided_dgrad_ksplit(2, 16, 20, 512, 1024, 1) == fused._conv_ksplit(2 * 8 * 10, 1024, 512, policy) == 4
    assert fused._strided_dgrad_ksplit(2, 800, 1334, 256, 128, 3) == 1   # (a full frame: enough workgroups as it is)
    prev = fused.set_conv_ksplit_policy(2048, 600, 2, 4)                  # the inference route's knob does not move this cut
    try:
        assert fused._strided_dgrad_ksplit(2, 16, 20, 256, 256, 3) == 4
    finally:
        fused.set_conv_ksplit_policy(*prev)
    assert fused._strided_dgrad_ksplit(1, 1, 1, 64, 64, 3) == 1    # (no odd pixel at all: still a valid number of pieces)


def test_switch_off_is_the_path_and_the_counts_of_before(monkeypatch):
    """CPU tensors are declined either way and nothing is counted; with the switch off backbone._conv_train does not hand a strided
    1 x 1 to conv_train at all, with it on it does."""
    from trackformer_amd import backbone, fused
    x = torch.randn(1, 8, 5, 6, requires_grad=True).contiguous(memory_format=torch.channels_last)
    w1 = torch.randn(64, 8, requires_grad=True)
    w3 = torch.randn(64, 72, requires_grad=True)
    calls = []
    monkeypatch.setattr(fused, "conv_train", lambda x, w, stride: calls.append((tuple(w.shape), stride)))
    proj = torch.nn.Conv2d(8, 64, 1, 2, bias=False)
    conv2 = torch.nn.Conv2d(8, 64, 3, 2, 1, bias=False)
    monkeypatch.setattr(backbone, "CHANNELS_LAST", True)
    for on in (False, True):
        prev = fused.set_strided_conv_training(on)
        try:
            before = fused.conv_train_counts()
            assert fused.strided_conv_training_enabled() is on
            calls.clear()
            backbone._conv_train(x, proj, proj.weight)
            backbone._conv_train(x, conv2, conv2.weight)
            assert calls == ([((64, 8), 2)] if on else []) + [((64, 72), 2)]
            assert fused.conv_train_counts() == before
        finally:
            fused.set_strided_conv_training(prev)
    monkeypatch.undo()
    before = fused.conv_train_counts()
    for on in (False, True):
        prev = fused.set_strided_conv_training(on)
        try:
            assert fused.conv_train(x, w1, 2) is None and fused.conv_train(x, w3, 2) is None
        finally:
            fused.set_strided_conv_training(prev)
    assert fused.conv_train_counts() == before
