"""tf_groupnorm_levels_nhwc_f32 (GroupNorm of several pyramid levels in two launches into one token buffer, csrc/fused_ops.hip) and
tf_conv_packed_partials_f32 (the convolution that leaves its split-K partial sums for it) on the CPU under the SIMT emulator, bound on
the emulated library itself.

Shapes at the kernels' edges: HW in {1, 63, 64, 65, 130} around the 64-row statistics block, (C, G) = (256, 32) and (288, 32) -- at 288 a
16-byte quad straddles two groups and 256 threads are no whole number of rows --, N = 1 and 2 under an image stride that is not
HW C, pieces in {1, 3, 5} (the reduce order's four-at-a-time loop and its remainder), mixed levels in one call whose output rows are
not in table order.  Checks: the float64 yardstick of tf_groupnorm_nhwc_f32 (tests/util_norm_attn_numerics.check, unchanged); BITWISE
equality with the numpy restatement of the kernels' summation order (tests/util_groupnorm_levels.restate); two calls equal bit for bit;
guard rows and the workspace behind its stated size untouched; refused arguments launch nothing."""
import ctypes

import numpy as np
import pytest
import torch

from tests import emu_lib
from tests import util_groupnorm_levels as GL
from tests import util_norm_attn_numerics as A

pytestmark = pytest.mark.skipif(not emu_lib.available(), reason="needs a host clang++ (ROCm's llvm) to build the emulated library")

EPS = 1e-5
CG = [(256, 32), (288, 32)]


def _backend():
    return GL.host_backend(emu_lib.lib())


def _check_level(got, lv, G, what):
    """Both yardsticks for one level: float64 bound (+ the fp32 formulation's own figure), bitwise restatement."""
    y = torch.from_numpy(lv["y"])
    gamma, beta = torch.from_numpy(lv["gamma"]), torch.from_numpy(lv["beta"])
    r = A.norm_reference([y], gamma, beta, EPS, G)
    A.check(torch.from_numpy(got), r, A.norm_fp32([y], gamma, beta, EPS, G), what)
    want = GL.restate(lv["y"], lv["gamma"], lv["beta"], G, EPS, lv["pieces"])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: differs from the restated arithmetic" % what


@pytest.mark.parametrize("C,G", CG, ids=["c256", "c288"])
@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("pieces", [1, 3, 5])
@pytest.mark.parametrize("HW", [1, 63, 64, 65, 130])
def test_one_level(HW, pieces, N, C, G):
    profile = A.NORM_PROFILES[(HW + pieces + N) % len(A.NORM_PROFILES)]
    lv = GL.make_level(profile, N, HW, C, G, pieces, seed=HW * 7 + pieces)
    rc, got, untouched, _ = GL.run_levels(_backend(), [lv], N, C, G, EPS)
    assert rc == 0
    _check_level(got[0], lv, G, "emu gn_levels %s HW %d pieces %d N %d C %d" % (profile, HW, pieces, N, C))
    assert untouched, "guard rows, the output's padding or the workspace behind its stated size were written (or a slot was not)"


@pytest.mark.parametrize("profile", ["offset3000", "offset300", "large", "chan_spread", "constant", "small_1e-6"])
@pytest.mark.parametrize("pieces", [1, 3])
def test_profiles_with_large_means(profile, pieces):
    """The profiles that lose the variance under fp32 sums of squares (|mean| up to 3000 std), over three statistics blocks."""
    N, HW, C, G = 2, 130, 256, 32
    lv = GL.make_level(profile, N, HW, C, G, pieces, seed=11 + pieces)
    rc, got, untouched, _ = GL.run_levels(_backend(), [lv], N, C, G, EPS)
    assert rc == 0 and untouched
    _check_level(got[0], lv, G, "emu gn_levels %s pieces %d" % (profile, pieces))


@pytest.mark.parametrize("C,G", CG, ids=["c256", "c288"])
@pytest.mark.parametrize("N", [1, 2])
def test_mixed_levels_in_one_call(N, C, G):
    """Five levels of every kind in one call; their output rows stand in another order than the table's (and not by size)."""
    spec = [(65, 1, "unit"), (1, 5, "offset30"), (130, 3, "offset3000"), (63, 1, "chan_spread"), (64, 5, "large")]
    levels = [GL.make_level(p, N, hw, C, G, pc, seed=100 + i, with_bias=(i != 1)) for i, (hw, pc, p) in enumerate(spec)]
    order = [3, 0, 4, 2, 1]
    rc, got, untouched, n_ws = GL.run_levels(_backend(), levels, N, C, G, EPS, order=order)
    assert rc == 0 and untouched
    slots = sum(-(-hw // GL.rows_per_block(pc, C)) for hw, pc, _p in spec)
    assert n_ws == N * slots * 2 * G
    for i, (lv, g) in enumerate(zip(levels, got)):
        _check_level(g, lv, G, "emu gn_levels mixed level %d %s N %d C %d" % (i, spec[i], N, C))
    rc2, got2, _, _ = GL.run_levels(_backend(), levels, N, C, G, EPS, order=order)
    assert rc2 == 0
    for a, b in zip(got, got2):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two calls on the same inputs differ"


def _conv_partials(x, w, bias, stride, ksplit):
    """tf_conv_packed_partials_f32 on the emulated library -> (pieces, partials [pieces', M * cout] with pieces' = max(ksplit, 1))."""
    L, up, _ = _backend()
    xa = emu_lib._aligned(x)
    n, h, wd, cin = xa.shape
    cout, ks = w.shape[0], w.shape[1]
    pk = emu_lib._packed(w.reshape(cout, ks * ks * cin))
    pad = 1 if ks == 3 else 0
    ho, wo = (h + 2 * pad - ks) // stride + 1, (wd + 2 * pad - ks) // stride + 1
    ws = emu_lib._aligned(np.full((max(ksplit, 1), n * ho * wo * cout), np.nan, np.float32))
    b = emu_lib._aligned(bias)
    pieces = ctypes.c_int(-1)
    rc = L.tf_conv_packed_partials_f32(emu_lib._p(xa), pk.ctypes.data, emu_lib._p(b), emu_lib._p(ws), ksplit, n, h, wd, cin, cout, ks, stride,
                                       emu_lib.TERMS, ctypes.byref(pieces), None)
    assert rc == 0, rc
    return pieces.value, ws, (n, ho * wo, cout)


@pytest.mark.parametrize("ks,stride,cin,ksplit", [(1, 1, 192, 3), (3, 2, 64, 5), (1, 1, 64, 1), (1, 1, 64, 64)],
                         ids=["1x1-3pieces", "3x3s2-5pieces", "unsplit", "ksplit-collapses"])
def test_deferred_reduce_partials_feed_the_levels(ks, stride, cin, ksplit):
    """The sibling entry runs the GEMM launch only: its piece count is what the launch code makes of ksplit, its partial sums added in z
    order plus the bias are the existing entry's output BIT FOR BIT (so is the y the statistics pass forms), and the levels call on
    those partials gives the restated arithmetic on that y.  Unsplit launches leave the finished y (pieces 1)."""
    prev = emu_lib.set_terms(16)
    try:
        g = np.random.default_rng(ks * 100 + cin)
        n, h, wd, cout, G = 2, 5, 7, 32, 8
        x = g.standard_normal((n, h, wd, cin), dtype=np.float32)
        w = (g.standard_normal((cout, ks, ks, cin)) / np.sqrt(ks * ks * cin)).astype(np.float32)
        bias = (0.1 * g.standard_normal(cout)).astype(np.float32)
        pieces, ws, (n_, hw, c) = _conv_partials(x, w, bias, stride, ksplit)
        assert pieces == GL.launch_pieces(ks * ks * cin, ksplit)
        y_ref = emu_lib.conv_packed(x, w, bias, stride=stride, ksplit=ksplit).reshape(n, hw, c)
        parts = ws[:pieces].reshape(pieces, n, hw, c)
        assert not np.isnan(parts).any()
        y = GL.reduce_y(parts, bias) if pieces > 1 else parts[0]
        assert np.array_equal(y.view(np.uint32), y_ref.view(np.uint32)), "the partial sums in z order + bias are not the reduce launch's y"
        gamma = (0.5 + g.random(c)).astype(np.float32)
        beta = (0.5 * g.standard_normal(c)).astype(np.float32)
        lv = dict(src=parts if pieces > 1 else parts[0], pieces=pieces, bias=bias if pieces > 1 else None, gamma=gamma, beta=beta, y=y_ref)
        rc, got, untouched, _ = GL.run_levels(_backend(), [lv], n, c, G, EPS)
        assert rc == 0 and untouched
        _check_level(got[0], lv, G, "emu gn_levels behind conv %dx%d s%d pieces %d" % (ks, ks, stride, pieces))
    finally:
        emu_lib.set_terms(prev)


def test_invalid_arguments_launch_nothing():
    L, up, _ = _backend()
    N, HW, C, G = 1, 5, 256, 32
    keep = [up(np.zeros((N, HW, C), np.float32)), up(np.ones(C, np.float32)), up(np.zeros(C, np.float32))]
    out, out_p = up(np.full((N, (HW + 1) * C), GL.SENTINEL, np.float32))
    ws, ws_p = up(np.full(4096, GL.WS_SENTINEL, np.float64))
    src_p, g_p, b_p = (k[1] for k in keep)

    def call(nl=1, src=src_p, gamma=g_p, beta=b_p, bias=None, pieces=1, hw=HW, row0=0, n=N, c=C, g=G, outp=out_p, stride=(HW + 1) * C, wsp=ws_p,
             table=True):
        t = (GL.GnLevel * 9)()
        for i in range(9):
            t[i].src, t[i].bias, t[i].gamma, t[i].beta, t[i].pieces, t[i].HW, t[i].row0 = src, bias, gamma, beta, pieces, hw, row0
        return L.tf_groupnorm_levels_nhwc_f32(t if table else None, nl, n, c, g, EPS, outp, stride, wsp, None)

    assert call() == 0
    assert not (out[:, :HW * C] == GL.SENTINEL).any()
    assert (ws[:2 * G] != GL.WS_SENTINEL).all() and (ws[2 * G:] == GL.WS_SENTINEL).all()
    out[...] = GL.SENTINEL
    ws[...] = GL.WS_SENTINEL
    NULLP, BAD = -1, -2
    assert call(table=False) == NULLP
    assert call(src=None) == NULLP
    assert call(gamma=None) == NULLP
    assert call(beta=None) == NULLP
    assert call(outp=None) == NULLP
    assert call(wsp=None) == NULLP
    assert call(nl=0) == BAD
    assert call(nl=9) == BAD                          # more than 8 levels
    assert call(nl=2) == BAD                          # two levels on the same output rows
    assert call(c=254) == BAD                         # C % 4
    assert call(c=256, g=48) == BAD                   # G does not divide C
    assert call(c=2048, g=32) == BAD
    assert call(g=512, c=1024) == BAD
    assert call(n=0) == BAD
    assert call(hw=0) == BAD
    assert call(pieces=0) == BAD
    assert call(row0=-1) == BAD
    assert call(row0=2) == BAD                        # rows behind the image stride
    assert call(stride=(HW + 1) * C + 2) == BAD       # stride % 4
    assert call(src=src_p + 4) == BAD                 # misaligned
    assert call(gamma=g_p + 8) == BAD
    assert call(beta=b_p + 4) == BAD
    assert call(bias=g_p + 4, pieces=1) == BAD
    assert call(outp=out_p + 8) == BAD
    assert call(wsp=ws_p + 8) == BAD
    assert call(src=out_p) == BAD                     # a source inside the output
    assert (out == GL.SENTINEL).all() and (ws == GL.WS_SENTINEL).all(), "a refused call wrote"
    t = (GL.GnLevel * 1)()
    t[0].src, t[0].gamma, t[0].beta, t[0].pieces, t[0].HW, t[0].row0 = src_p, g_p, b_p, 1, HW, 0
    assert L.tf_groupnorm_levels_workspace_doubles(t, 1, N, C, G) == 2 * G
    assert L.tf_groupnorm_levels_workspace_doubles(t, 1, N, 254, G) == -1
    # the convolution sibling: its own two pointers, then tf_conv_packed_f32's checks
    one = ctypes.c_int(0)
    fn = L.tf_conv_packed_partials_f32
    assert fn(src_p, src_p, None, None, 2, 1, 4, 4, 64, 32, 1, 1, 16, ctypes.byref(one), None) == NULLP
    assert fn(src_p, src_p, None, ws_p, 2, 1, 4, 4, 64, 32, 1, 1, 16, None, None) == NULLP
    assert fn(src_p, src_p, None, ws_p + 4, 2, 1, 4, 4, 64, 32, 1, 1, 16, ctypes.byref(one), None) == BAD
    assert fn(src_p, src_p, None, ws_p, 2, 1, 4, 4, 64, 30, 1, 1, 16, ctypes.byref(one), None) == BAD
    assert fn(src_p, src_p, None, ws_p, 65, 1, 4, 4, 64, 32, 1, 1, 16, ctypes.byref(one), None) == BAD
    assert (ws == GL.WS_SENTINEL).all()
