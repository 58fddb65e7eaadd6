"""tf_linear_groups_f32 (several projections of one token tile in one launch, csrc/ffn_fused.hip) on the CPU under the SIMT emulator:
every group's output must equal, BIT FOR BIT, what the emulated tf_linear_split_f32 (groups of x) / tf_linear_split_add_f32 (groups of
x + x2) compute -- every kernel instantiation that is built (fp16 pieces with 32-, 64- and 96-row blocks, forced through the option
"groups_ti": without it these row counts would only reach the 32-row kernel; six terms with the 32-row blocks it has), rows below one
tile / one tile + 1 / two tiles + a tail of the 96-row tile, full and narrow column chunks, with and without bias, dynamic LDS
poisoned (the emulator's default), guard rows behind row M untouched."""
import numpy as np
import pytest

from tests import emu_lib
from trackformer_amd import _cabi

pytestmark = pytest.mark.skipif(not emu_lib.available(), reason="needs a host clang++ (ROCm's llvm) to build the emulated library")

K = 256
GUARD = 3
# (output width, add_x2) per group
GROUP_LISTS = {
    "256": [(256, False)],
    "384add": [(384, True)],
    "256_384add": [(256, False), (384, True)],
    "256x6": [(256, False)] * 6,
    "256_128": [(256, False), (128, False)],
}


ProjGroup = _cabi.ProjGroup


def linear_groups(x, x2, groups, guard_rows=GUARD):
    """groups: [(w [N, 256], bias | None, add)] -> (status, [y with guard_rows NaN-pattern rows behind row M])."""
    x = emu_lib._aligned(x)
    x2 = emu_lib._aligned(x2)
    M = x.shape[0]
    keep, descs, ys = [], (ProjGroup * len(groups))(), []
    for d, (w, b, add) in zip(descs, groups):
        pk, b = emu_lib._packed(w), emu_lib._aligned(b)
        y = emu_lib._aligned(np.full((M + guard_rows, w.shape[0]), np.nan, np.float32))
        keep += [pk, b]
        ys.append(y)
        d.w_packed, d.bias, d.y, d.N, d.add_x2 = pk.ctypes.data, emu_lib._p(b), y.ctypes.data, w.shape[0], int(add)
    rc = emu_lib.lib().tf_linear_groups_f32(emu_lib._p(x), emu_lib._p(x2), descs, len(groups), M, x.shape[1], emu_lib.TERMS, None)
    return rc, ys


_DATA = {}


def _data(M):
    """Inputs and weights for M rows, made once and left unchanged (the references below are cached per (terms, M, group, bias))."""
    if M not in _DATA:
        g = np.random.default_rng(1000 + M)
        x = g.standard_normal((M, K), dtype=np.float32)
        x2 = (0.5 * g.standard_normal((M, K))).astype(np.float32)
        ws = [(g.standard_normal((n, K)) / 16).astype(np.float32) * np.exp2(g.integers(-3, 4, (n, 1))).astype(np.float32) for n in (256, 384, 128)]
        ws += [(g.standard_normal((256, K)) / 16).astype(np.float32) for _ in range(5)]   # the other five 256-wide weights of "256x6"
        bs = [(0.1 * g.standard_normal(w.shape[0])).astype(np.float32) for w in ws]
        _DATA[M] = (x, x2, ws, bs)
    return _DATA[M]


_REF = {}


def _reference(terms, M, wi, add, with_bias):
    key = (terms, M, wi, add, with_bias)
    if key not in _REF:
        x, x2, ws, bs = _data(M)
        b = bs[wi] if with_bias else None
        _REF[key] = emu_lib.linear_split_add(x, x2, ws[wi], b) if add else emu_lib.linear_split(x, ws[wi], b)
    return _REF[key]


def _weights_of(name):
    """Indices into _data()'s weight list for a group list: 256 -> 0 (then 3.. for repeats), 384 -> 1, 128 -> 2."""
    out, n256 = [], 0
    for n, _add in GROUP_LISTS[name]:
        if n == 256:
            out.append(0 if n256 == 0 else 2 + n256)
            n256 += 1
        else:
            out.append(1 if n == 384 else 2)
    return out


# (terms, groups_ti): linear_groups_kernel<16, 1 | 2 | 3> (32 / 64 / 96 rows per block; 96 is what the full-size frame runs) and <3, 1>
VARIANTS = [(16, 1), (16, 2), (16, 3), (6, 0)]


@pytest.mark.parametrize("terms,ti", VARIANTS, ids=["f16-32rows", "f16-64rows", "f16-96rows", "six-32rows"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("name", list(GROUP_LISTS))
@pytest.mark.parametrize("M", [1, 33, 97, 200])
def test_groups_bit_identical_to_separate_kernels(M, name, with_bias, terms, ti):
    prev = emu_lib.set_terms(terms)
    prev_opt = emu_lib.set_options(groups_ti=ti)
    try:
        x, x2, ws, bs = _data(M)
        idx = _weights_of(name)
        groups = [(ws[wi], bs[wi] if with_bias else None, add) for wi, (_n, add) in zip(idx, GROUP_LISTS[name])]
        rc, ys = linear_groups(x, x2, groups)
        assert rc == 0
        for wi, (n, add), y in zip(idx, GROUP_LISTS[name], ys):
            ref = _reference(terms, M, wi, add, with_bias)
            assert y.shape == (M + GUARD, n)
            assert np.array_equal(y[:M].view(np.uint32), ref.view(np.uint32)), "group %d x %s differs from the separate kernel" % (n, add)
            assert np.isnan(y[M:]).all(), "rows behind M were written"
    finally:
        emu_lib.set_options(**prev_opt)
        emu_lib.set_terms(prev)


def test_groups_ti_option_selects_the_kernel_and_restores():
    """The option is what the cases above rely on: it returns the previous value, takes values outside 1..3 as 0 (by row count), and
    decides how many workgroups a launch runs: 200 rows are 7 / 4 / 3 blocks of 32 / 64 / 96 rows (the packing of the weight
    launches the same small kernels in every call: the counts are compared with each other)."""
    prev = emu_lib.set_terms(16)
    first = emu_lib.set_options(groups_ti=0)
    try:
        x, x2, ws, bs = _data(200)
        blocks = {}
        for ti in (0, 1, 2, 3):
            emu_lib.set_options(groups_ti=ti)
            emu_lib.stats(reset=True)
            rc, _ys = linear_groups(x, x2, [(ws[2], bs[2], False)])
            assert rc == 0
            blocks[ti] = emu_lib.stats(reset=True)["blocks"]
        assert blocks[1] - blocks[2] == 7 - 4 and blocks[1] - blocks[3] == 7 - 3 and blocks[0] == blocks[1], blocks
        assert emu_lib.set_options(groups_ti=7)["groups_ti"] == 3      # the value set last in the loop
        assert emu_lib.set_options(groups_ti=2)["groups_ti"] == 0      # 7 was taken as 0
        assert emu_lib.set_options(groups_ti=0)["groups_ti"] == 2
    finally:
        emu_lib.set_options(**first)
        emu_lib.set_terms(prev)


def test_groups_order_of_the_caller_is_kept_when_kinds_interleave():
    """[384 of x + x2, 256 of x]: the kernel runs the x groups first; each output still lands in its own group's buffer."""
    prev = emu_lib.set_terms(16)
    try:
        x, x2, ws, bs = _data(97)
        rc, ys = linear_groups(x, x2, [(ws[1], bs[1], True), (ws[0], bs[0], False)])
        assert rc == 0
        assert np.array_equal(ys[0][:97].view(np.uint32), _reference(16, 97, 1, True, True).view(np.uint32))
        assert np.array_equal(ys[1][:97].view(np.uint32), _reference(16, 97, 0, False, True).view(np.uint32))
    finally:
        emu_lib.set_terms(prev)


def test_groups_width_that_is_no_multiple_of_128():
    """N = 160: one narrow chunk whose last three tiles are the image's padding -- computed, never stored."""
    prev = emu_lib.set_terms(16)
    try:
        x, x2, ws, bs = _data(33)
        w, b = np.ascontiguousarray(ws[1][:160]), np.ascontiguousarray(bs[1][:160])
        rc, ys = linear_groups(x, x2, [(w, b, False)])
        assert rc == 0
        assert np.array_equal(ys[0][:33].view(np.uint32), emu_lib.linear_split(x, w, b).view(np.uint32))
        assert np.isnan(ys[0][33:]).all()
    finally:
        emu_lib.set_terms(prev)


def test_groups_invalid_arguments_launch_nothing():
    x, x2, ws, bs = _data(33)
    fn = emu_lib.lib().tf_linear_groups_f32
    xa, x2a = emu_lib._aligned(x), emu_lib._aligned(x2)
    pk = emu_lib._packed(ws[0])
    y = emu_lib._aligned(np.full((33, 256), np.nan, np.float32))
    T = emu_lib.TERMS

    def call(xp=None, x2p=None, w=pk.ctypes.data, yp=y.ctypes.data, N=256, add=0, ng=1, M=33, Kk=K, terms=T):
        d = (ProjGroup * 9)()
        for i in range(9):
            d[i].w_packed, d[i].bias, d[i].y, d[i].N, d[i].add_x2 = w, None, yp, N, add
        return fn(xa.ctypes.data if xp is None else xp, x2p, d, ng, M, Kk, terms, None)

    assert call() == 0
    assert np.isfinite(y).all()
    y[...] = np.nan
    NULLP, BAD = -1, -2
    assert call(xp=0) == NULLP
    assert call(w=None) == NULLP
    assert call(yp=None) == NULLP
    assert call(add=1) == NULLP                       # add_x2 without x2
    assert call(add=1, x2p=x2a.ctypes.data) == 0
    y[...] = np.nan
    assert call(ng=0) == BAD
    assert call(ng=9) == BAD
    assert call(M=0) == BAD
    assert call(Kk=288) == BAD                        # hidden 288: not built, the caller keeps the separate launches
    assert call(Kk=128) == BAD
    assert call(terms=3) == BAD
    assert call(N=250) == BAD                         # N % 32
    assert call(N=0) == BAD
    assert call(xp=xa.ctypes.data + 4) == BAD         # misaligned
    assert call(yp=y.ctypes.data + 8) == BAD
    assert call(w=pk.ctypes.data + 2) == BAD
    assert np.isnan(y).all(), "a refused call wrote to y"
