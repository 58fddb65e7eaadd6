"""GPU: tf_linear_groups_f32 / fused.linear_groups (several projections of one token tile in one launch) against the launches it
replaces -- tf_linear_split_f32 for the groups of x, tf_linear_split_add_f32 for the groups of x + x2 -- BIT FOR BIT: both split
schemes, rows below / at / across the 32- and 96-row tiles and across the threshold between the two block sizes (4096), sentinel
rows behind row M, non-finite rows, weight updates (eagerly and under a captured graph), a small transformer with the route on and
off, and refused arguments."""

import pytest
import torch
from torch import nn

from tests import util_weight_coherence as wc
from trackformer_amd import _cabi, fused
from trackformer_amd import deformable_transformer as dt

pytestmark = pytest.mark.gpu

K = 256
GUARD = 5
SENTINEL = -1234.5
GROUP_LISTS = {
    "256": [(256, False)],
    "384add": [(384, True)],
    "256_384add": [(256, False), (384, True)],
    "256x6": [(256, False)] * 6,
    "256_128": [(256, False), (128, False)],
}
ROWS = [1, 97, 200, 4099]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    _cabi.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def data(dev):
    """Inputs (the largest row count; smaller cases take its first rows) and weights, made once and left unchanged."""
    g = torch.Generator().manual_seed(17)
    x = torch.randn(max(ROWS), K, generator=g)
    x2 = 0.5 * torch.randn(max(ROWS), K, generator=g)
    ws = {n: [(torch.randn(n, K, generator=g) / 16 * torch.exp2(torch.randint(-3, 4, (n, 1), generator=g).float())).to(dev)
              for _ in range(6 if n == 256 else 1)] for n in (256, 384, 128)}
    bs = {n: [(0.1 * torch.randn(n, generator=g)).to(dev) for _ in ws[n]] for n in ws}
    return x.to(dev), x2.to(dev), ws, bs


def _pick(ws, bs, name, with_bias=True):
    out, seen = [], {}
    for n, add in GROUP_LISTS[name]:
        i = seen.get(n, 0)
        seen[n] = i + 1
        out.append((ws[n][i], bs[n][i] if with_bias else None, add))
    return out


def _reference(x, x2, w, b, add):
    """The separate kernel of the group's kind, called directly (not through fused.linear, which may pick another kernel)."""
    hi, mid, lo, wsc = fused._split_weight(w)
    M = x.shape[0]
    y = torch.empty((M, w.shape[0]), dtype=torch.float32, device=x.device)
    L, s = _cabi.lib(), torch.cuda.current_stream(x.device).cuda_stream
    p = lambda t: 0 if t is None else t.data_ptr()
    if add:
        rc = L.tf_linear_split_add_f32(x.data_ptr(), x2.data_ptr(), hi.data_ptr(), mid.data_ptr(), p(lo), p(wsc), p(b), y.data_ptr(), M, K,
                                       w.shape[0], s)
    else:
        rc = L.tf_linear_split_f32(x.data_ptr(), hi.data_ptr(), mid.data_ptr(), p(lo), p(wsc), p(b), y.data_ptr(), M, K, w.shape[0], 0, s)
    assert rc == 0
    return y


def _grouped(x, x2, groups, guard=GUARD):
    """tf_linear_groups_f32 directly, every output with `guard` sentinel rows behind row M -> (status, outputs incl. guard rows)."""
    M = x.shape[0]
    descs = (_cabi.ProjGroup * len(groups))()
    ys, keep = [], []
    for d, (w, b, add) in zip(descs, groups):
        pk = fused._packed_weight(w, None)
        y = torch.full((M + guard, w.shape[0]), SENTINEL, dtype=torch.float32, device=x.device)
        keep.append(pk)
        ys.append(y)
        d.w_packed, d.bias, d.y, d.N, d.add_x2 = pk.data_ptr(), (b.data_ptr() if b is not None else None), y.data_ptr(), w.shape[0], int(add)
    rc = _cabi.lib().tf_linear_groups_f32(x.data_ptr(), x2.data_ptr(), descs, len(groups), M, K, fused.split_terms(),
                                          torch.cuda.current_stream(x.device).cuda_stream)
    torch.cuda.synchronize()
    return rc, ys


def _bits(t):
    return t.contiguous().view(torch.int32)


# (terms, option "groups_ti"): every instantiation that is built -- fp16 pieces with 32 / 64 / 96 rows per block at EVERY row count
# (by itself the entry takes 32 rows below 4096 rows and 96 from there on), six terms with the 32-row blocks they have
VARIANTS = [(16, 1), (16, 2), (16, 3), (16, 0), (6, 0)]


@pytest.mark.parametrize("terms,ti", VARIANTS, ids=["f16-32rows", "f16-64rows", "f16-96rows", "f16-auto", "six-32rows"])
@pytest.mark.parametrize("name", list(GROUP_LISTS))
@pytest.mark.parametrize("M", ROWS)
def test_groups_equal_the_separate_kernels_bit_for_bit(dev, data, M, name, terms, ti):
    x, x2, ws, bs = data
    x, x2 = x[:M].contiguous(), x2[:M].contiguous()
    prev = fused.set_split_terms(terms)
    prev_ti = _cabi.lib().tf_msda_set_option(b"groups_ti", ti)
    try:
        for with_bias in (True, False):
            groups = _pick(ws, bs, name, with_bias)
            rc, ys = _grouped(x, x2, groups)
            assert rc == 0
            for (w, b, add), y in zip(groups, ys):
                assert torch.equal(_bits(y[:M]), _bits(_reference(x, x2, w, b, add))), (name, w.shape[0], add, with_bias)
                assert bool((y[M:] == SENTINEL).all()), "rows behind M were written"
    finally:
        _cabi.lib().tf_msda_set_option(b"groups_ti", prev_ti)
        fused.set_split_terms(prev)


@pytest.mark.parametrize("terms,ti", [(16, 1), (16, 3), (6, 0)], ids=["f16-32rows", "f16-96rows", "six-32rows"])
def test_rows_with_nan_and_inf_equal_the_separate_kernels(dev, data, terms, ti):
    x, x2, ws, bs = data
    M = 200
    x, x2 = x[:M].clone(), x2[:M].clone()
    x[3, 7] = float("nan")
    x[40, 0] = float("inf")
    x[41, 255] = float("-inf")
    x2[41, 255] = float("inf")      # inf - inf in the sum
    x2[100, 31] = float("nan")
    x[150, 9] = 3.0e38
    x2[150, 9] = 3.0e38             # the sum overflows
    x[199, 128] = 2.0e6             # beyond the fp16 scheme's activation range
    prev = fused.set_split_terms(terms)
    prev_ti = _cabi.lib().tf_msda_set_option(b"groups_ti", ti)
    try:
        groups = _pick(ws, bs, "256_384add")
        rc, ys = _grouped(x, x2, groups)
        assert rc == 0
        for (w, b, add), y in zip(groups, ys):
            ref = _reference(x, x2, w, b, add)
            assert not bool(torch.isfinite(ref).all()), "the case holds no non-finite output"
            nan = torch.isnan(ref)
            assert torch.equal(torch.isnan(y[:M]), nan)
            assert torch.equal(_bits(y[:M])[~nan], _bits(ref)[~nan])     # (equal_nan: NaN where the reference has NaN, else the same bits)
            assert bool((y[M:] == SENTINEL).all())
    finally:
        _cabi.lib().tf_msda_set_option(b"groups_ti", prev_ti)
        fused.set_split_terms(prev)


class _Pair(nn.Module):
    """The encoder layer's pair through fused.linear_groups: value (x) and query (x + x2) projections."""

    def __init__(self):
        super().__init__()
        self.value, self.query = nn.Linear(K, 256), nn.Linear(K, 384)

    def forward(self, x, x2):
        ys = fused.linear_groups(x, x2, [(self.value.weight, self.value.bias, False), (self.query.weight, self.query.bias, True)])
        assert ys is not None, "fused.linear_groups declined the call"
        return ys


@pytest.fixture()
def low_threshold():
    prev = fused.set_proj_groups_min_rows(1)
    yield
    fused.set_proj_groups_min_rows(prev)


def _cold(m, x, x2):
    """The separate kernels on pieces built from clones of the CURRENT parameters: no cached image involved."""
    return [_reference(x, x2, m.value.weight.detach().clone(), m.value.bias.detach().clone(), False),
            _reference(x, x2, m.query.weight.detach().clone(), m.query.bias.detach().clone(), True)]


@pytest.mark.parametrize("target", ["value.weight", "query.weight", "query.bias"])
def test_an_in_place_weight_update_reaches_the_next_call(dev, data, low_threshold, target):
    x, x2 = data[0][:97].contiguous(), data[1][:97].contiguous()
    m = wc.randomize(_Pair(), seed=3).to(dev)
    with torch.no_grad():
        before = [y.clone() for y in m(x, x2)]
        assert wc.bits_equal(before, _cold(m, x, x2))
        wc.mut_inplace(m, target)
        after = [y.clone() for y in m(x, x2)]
    assert wc.bits_equal(after, _cold(m, x, x2)), "a stale weight image"
    assert not wc.bits_equal(after, before), "the update changed nothing: the case tests nothing"


def test_a_graph_captured_after_the_update_replays_the_new_weights(dev, data, low_threshold):
    """Captured graphs bake the addresses of the weight images, and an update makes NEW images at new addresses: a graph captured before
    the update cannot follow it by design (replaying it reads the old, by then released, image) -- whoever holds a graph drops it
    when a weight changes (GraphedDetector does, tests/test_weight_coherence_gpu.py) and captures again.  That is the case here: the
    graph captured after the update must replay the new weights.  Inside a capture no image is ever built: with one missing the call
    declines (the caller takes the separate kernels)."""
    x, x2 = data[0][:200].contiguous(), data[1][:200].contiguous()
    m = wc.randomize(_Pair(), seed=4).to(dev)

    def captured():
        graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(graph):
            ys = m(x, x2)
        return graph, ys
    with torch.no_grad():
        m(x, x2)                                     # the images exist before the capture
        torch.cuda.synchronize()
        g1, ys1 = captured()
        g1.replay()
        torch.cuda.synchronize()
        before = [y.clone() for y in ys1]
        assert wc.bits_equal(before, _cold(m, x, x2))
        wc.mut_inplace(m, "value.weight")
        wc.mut_inplace(m, "query.weight")
        torch.cuda.synchronize()
        probe = torch.cuda.CUDAGraph()
        with torch.cuda.graph(probe):                # a real capture while the images of the new weights are missing
            other = x[:1] + 1.0                      # (so that the graph is not empty)
            declined = fused.linear_groups(x, x2, [(m.value.weight, m.value.bias, False)])
        assert declined is None, "an image was built inside a capture"
        assert not m.value.weight._tf_packed[1], "an image was cached inside a capture"
        del probe, other
        m(x, x2)                                     # eagerly: the new images
        torch.cuda.synchronize()
        g2, ys2 = captured()
        g2.replay()
        torch.cuda.synchronize()
        after = [y.clone() for y in ys2]
    assert wc.bits_equal(after, _cold(m, x, x2)), "the graph captured after the update replays a stale weight image"
    assert not wc.bits_equal(after, before)


def _transformer_run(tr, inputs):
    srcs, masks, pos, query = inputs
    with torch.no_grad():
        hs, memory, _init, inter, _a, _b = tr(srcs, masks, pos, query)
    return [memory.clone(), hs.clone(), inter.clone()]


@pytest.mark.parametrize("padded", [False, True], ids=["unpadded", "padded"])
def test_small_transformer_is_bit_identical_with_the_route_on_and_off(dev, low_threshold, padded):
    """Hidden 256, two levels (12 x 16, 6 x 8: 240 tokens), two encoder and two decoder layers: encoder memory, decoder hs and the
    references with both grouped routes on equal those with both off, bit for bit (padded: the padding mask's masked_fill on every
    value slice)."""
    g = torch.Generator().manual_seed(23)
    tr = dt.DeformableTransformer(d_model=256, nhead=8, num_encoder_layers=2, num_decoder_layers=2, dim_feedforward=64, dropout=0.0,
                                  return_intermediate_dec=True, num_feature_levels=2)
    tr = wc.randomize(tr, seed=6).to(dev)
    shapes = ((12, 16), (6, 8))
    srcs = [torch.randn(1, 256, h, w, generator=g).to(dev) for h, w in shapes]
    pos = [torch.randn(1, 256, h, w, generator=g).to(dev) for h, w in shapes]
    masks = [torch.zeros(1, h, w, dtype=torch.bool, device=dev) for h, w in shapes]
    if padded:
        for mk in masks:
            mk[:, :, -(mk.shape[2] // 4):] = True
    query = torch.randn(9, 512, generator=g).to(dev)
    inputs = (srcs, masks, pos, query)
    calls = {"n": 0}
    real = fused.linear_groups

    def counted(*a, **k):
        y = real(*a, **k)
        calls["n"] += y is not None
        return y
    prev = fused.set_proj_groups(True)
    fused.linear_groups = counted
    try:
        on = _transformer_run(tr, inputs)
        assert calls["n"] == 2 + 1, "the grouped launches did not run (2 encoder layers + 1 for the decoder): %d" % calls["n"]
        fused.set_proj_groups(False)
        off = _transformer_run(tr, inputs)
        assert calls["n"] == 3
        fused.set_proj_groups("enc")
        enc_only = _transformer_run(tr, inputs)
        assert calls["n"] == 5
    finally:
        fused.linear_groups = real
        fused.set_proj_groups(prev)
    assert wc.bits_equal(on, off)
    assert wc.bits_equal(enc_only, off)


def test_invalid_arguments_return_error_codes_and_launch_nothing(dev, data):
    x, x2, ws, bs = data
    x, x2 = x[:33].contiguous(), x2[:33].contiguous()
    w = ws[256][0]
    pk = fused._packed_weight(w, None)
    y = torch.full((33 + GUARD, 256), SENTINEL, dtype=torch.float32, device=dev)
    fn = _cabi.lib().tf_linear_groups_f32
    s = torch.cuda.current_stream(dev).cuda_stream

    def call(xp=x.data_ptr(), x2p=None, wp=pk.data_ptr(), yp=y.data_ptr(), N=256, add=0, ng=1, M=33, Kk=K, terms=16):
        d = (_cabi.ProjGroup * 9)()
        for i in range(9):
            d[i].w_packed, d[i].bias, d[i].y, d[i].N, d[i].add_x2 = wp, None, yp, N, add
        return fn(xp, x2p, d, ng, M, Kk, terms, s)
    NULLP, BAD = -1, -2
    prev = fused.set_split_terms(16)
    try:
        assert call(xp=None) == NULLP
        assert call(wp=None) == NULLP
        assert call(yp=None) == NULLP
        assert call(add=1) == NULLP                      # add_x2 without x2
        assert call(ng=0) == BAD and call(ng=9) == BAD
        assert call(M=0) == BAD
        assert call(Kk=288) == BAD and call(Kk=128) == BAD
        assert call(terms=3) == BAD
        assert call(N=250) == BAD and call(N=0) == BAD
        assert call(N=4096, ng=2) == BAD                 # more columns than the kernel's bias / scale tables hold
        assert call(xp=x.data_ptr() + 4) == BAD          # misaligned
        assert call(yp=y.data_ptr() + 8) == BAD
        assert call(wp=pk.data_ptr() + 2) == BAD
        assert call(add=1, x2p=x2.data_ptr() + 4) == BAD
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all()), "a refused call wrote to y"
        assert call() == 0
        torch.cuda.synchronize()
        assert bool((y[:33] != SENTINEL).any()) and bool((y[33:] == SENTINEL).all())
    finally:
        fused.set_split_terms(prev)
