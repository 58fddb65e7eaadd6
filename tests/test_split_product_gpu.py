"""GPU (-m gpu): every entry point that includes csrc/split_product.h, in both split products (six bf16 terms, fp16 pieces) and every
magnitude profile of tests/util_split_numerics.py, against float64 with the yardstick there: (|y - ref| - floor) / S <= 2^-20 and
within four times torch's fp32 error; the non-finite contract (a NaN or an over-limit activation makes exactly the outputs that read it
NaN) through ReLU, the fused feed-forward block's hidden layer and the LayerNorm epilogues.  Shapes at the kernels' edges: one row,
ragged row and column tails, the dispatch thresholds, split-K pieces that do not divide K.  Each case prints its largest normalised
excess ("EXCESS <entry> <scheme> <profile> <value>"): the measurement of both products on the chip."""
import pytest
import torch
import torch.nn.functional as F

from tests import util_split_numerics as U

pytestmark = pytest.mark.gpu

PROFILES = U.PROFILES + ["nonfinite"]
SCHEMES = [16, 6]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    from trackformer_amd import _cabi
    _cabi.lib()
    return torch.device("cuda:0")


@pytest.fixture(params=SCHEMES, ids=["fp16_pieces", "six_terms"])
def terms(request):
    from trackformer_amd import fused
    prev_on, prev = fused.set_split_linear(True), fused.set_split_terms(request.param)
    prev_check = fused.set_check_finite(False)
    try:
        yield request.param
    finally:
        fused.set_check_finite(prev_check)
        fused.set_split_terms(prev)
        fused.set_split_linear(prev_on)


def _report(entry, terms, profile, worst):
    print("EXCESS %-22s %-11s %-14s %.3e  (fp32 %.3e)" % (entry, "fp16_pieces" if terms == 16 else "six_terms", profile, worst.value,
                                                          worst.fp32_err))


def _check_linear(entry, terms, profile, y, x, w, b=None, r=None, relu=False):
    ref, S, floor, nan = U.linear_reference(x, w, b, r, relu, terms)
    worst = U.check(y.reshape(ref.shape), ref, S, floor, nan, fp32=U.linear_fp32(x, w, b, r, relu))
    _report(entry, terms, profile, worst)
    return worst


def _option(name, value):
    from trackformer_amd import _cabi
    return _cabi.lib().tf_msda_set_option(name.encode(), value)


# ---- linears -------------------------------------------------------------------------------------------------------------------------
LINEAR = [(1, 32, 1, False, False), (33, 96, 200, True, True), (4097, 288, 96, False, True), (33, 1152, 200, True, False),
          (4096, 32, 96, True, True)]   # M, K, N, residual, relu


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("M,K,N,res,relu", LINEAR, ids=["%dx%dx%d" % s[:3] for s in LINEAR])
def test_split_linear(dev, terms, profile, M, K, N, res, relu):
    """tf_linear_split_f32 / tf_linear_split_res_f32 (the LDS-staged block kernel; split_gemm_deep for few rows)."""
    from trackformer_amd import fused
    x, w, b, r = U.linear_operands(profile, M, K, N, seed=M + K + N, device=dev, residual=res)
    prev = fused.set_packed_linear(False)
    try:
        y = fused.linear(x, w, b, relu=relu, residual=r)
    finally:
        fused.set_packed_linear(prev)
    assert y is not None and y.shape == (M, N)
    _check_linear("linear_split", terms, profile, y, x, w, b, r, relu)


PACKED = [(4097, 256, 256), (4225, 128, 96), (4161, 64, 400)]   # N mod 256: 0, <= 128, > 128


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("M,K,N", PACKED, ids=["%dx%dx%d" % s for s in PACKED])
def test_packed_linear(dev, terms, profile, M, K, N, monkeypatch):
    """tf_linear_packed_f32 (stream_gemm) with residual + ReLU, M just above _PACKED_MIN_ROWS and not a multiple of 128."""
    from trackformer_amd import fused
    assert M > fused._PACKED_MIN_ROWS
    monkeypatch.setattr(fused, "_use_packed", lambda m, k, n: k % 64 == 0)
    x, w, b, r = U.linear_operands(profile, M, K, N, seed=M + N, device=dev, residual=True)
    y = fused.linear(x, w, b, relu=True, residual=r)
    assert y is not None and getattr(w, "_tf_packed", None) is not None
    _check_linear("linear_packed", terms, profile, y, x, w, b, r, True)


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_lds_dma_gemm_is_bit_identical_to_the_stream_form(dev, terms, profile, mode, monkeypatch):
    """The opt-in linear_dma modes of tf_linear_packed_f32: the bits of the stream form in every profile."""
    from trackformer_amd import fused
    monkeypatch.setattr(fused, "_use_packed", lambda m, k, n: k % 64 == 0)
    M, K, N = 513, 192, 384
    x, w, b, r = U.linear_operands(profile, M, K, N, seed=mode, device=dev, residual=True)
    prev = _option("linear_dma", 0)
    try:
        want = fused.linear(x, w, b, relu=True, residual=r)
        _option("linear_dma", mode)
        got = fused.linear(x, w, b, relu=True, residual=r)
    finally:
        _option("linear_dma", prev)
    assert torch.equal(got.isnan(), want.isnan()) and torch.equal(got.nan_to_num(), want.nan_to_num())
    _check_linear("linear_dma%d" % mode, terms, profile, got, x, w, b, r, True)


ADD = [(300, 256, 384), (5000, 256, 384), (4500, 256, 256), (130, 288, 288)]


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("M,K,N", ADD, ids=["%dx%dx%d" % s for s in ADD])
def test_linear_split_add(dev, terms, profile, M, K, N):
    """tf_linear_split_add_f32: (x + pos) w^T + b against float64 of (x + pos); S from |x| + |pos| (the prologue's fp32 add rounds)."""
    from trackformer_amd import fused
    x, w, b, _ = U.linear_operands(profile, M, K, N, seed=M + N, device=dev)
    pos, _, _, _ = U.linear_operands("unit" if profile in ("nonfinite", "large_x") else profile, M, K, N, seed=M + N + 1, device=dev)
    y = fused.linear_add(x, pos, w, b)
    assert y is not None
    ref, _, _, nan = U.linear_reference(x.double() + pos.double(), w, b, terms=terms)
    _, S, _, _ = U.linear_reference(x.abs() + pos.abs(), w, b, terms=terms)
    floor = U.small_floor(x + pos, w, terms)
    worst = U.check(y, ref, S, floor, nan, fp32=U.linear_fp32(x + pos, w, b))
    _report("linear_split_add", terms, profile, worst)


# ---- linear + residual + LayerNorm, the fused feed-forward block -----------------------------------------------------------------------
def _norm(D, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.1 * torch.randn(D, generator=g)).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev)


def _module(w, b):
    lin = torch.nn.Linear(w.shape[1], w.shape[0]).to(w.device)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
    return lin


def _check_ln(entry, terms, profile, y, pre, S, floor, nan, gamma, beta, eps, keep=None):
    ref, Sn, fn, nan_n = U.layernorm_reference(pre, S, floor, gamma, beta, eps, nan)
    if keep is not None:
        y, ref, Sn, fn, nan_n = y[keep], ref[keep], Sn[keep], fn[keep], nan_n[keep]
    worst = U.check(y, ref, Sn, fn, nan_n)
    _report(entry, terms, profile, worst)


LINLN = [(256, 256, 0), (256, 288, 1), (257, 256, 2), (1000, 288, 3)]   # M, D, linln_ti


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("M,D,ti", LINLN, ids=["%dx%d_ti%d" % s for s in LINLN])
def test_linear_residual_layernorm(dev, terms, profile, M, D, ti, monkeypatch):
    """tf_linear_res_ln_f32: LayerNorm(r + x w^T + b) against float64 with the norm-aware bound."""
    from trackformer_amd import fused
    monkeypatch.setattr(fused, "_LINLN_MIN_ROWS", 256)
    x, w, b, r = U.linear_operands(profile, M, D, D, seed=M + D + ti, device=dev, residual=True)
    gamma, beta = _norm(D, dev, ti)
    lin, norm = _module(w, b), torch.nn.LayerNorm(D).to(dev)
    with torch.no_grad():
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    prev_on, prev_ti = fused.set_linear_ln_fused(True), _option("linln_ti", ti)
    try:
        with torch.no_grad():
            y = fused.linear_residual_norm(x, lin, r, norm)
    finally:
        fused.set_linear_ln_fused(prev_on)
        _option("linln_ti", prev_ti)
    assert y is not None
    pre, S, floor, nan = U.linear_reference(x, w, b, r, terms=terms)
    _check_ln("linear_res_ln", terms, profile, y, pre, S, floor, nan, gamma, beta, 1e-5)


def _ffn_rows_tail():
    """Rows that turn on the tail split of the 64-row FFN blocks: one full round of 64 * CUs rows plus 44 (less than half a round)."""
    return 64 * torch.cuda.get_device_properties(0).multi_processor_count + 44


FFN = [(256, 1024, 3, "tail", True), (288, 1024, 2, 4100, False), (256, 128, 1, 4096, True), (288, 160, 1, 4100, True)]


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("D,Fd,ti,M,ln", FFN, ids=["d%d_f%d_ti%d_%s_%s" % (s[0], s[1], s[2], s[3], "ln" if s[4] else "plain") for s in FFN])
def test_fused_ffn(dev, terms, profile, D, Fd, ti, M, ln, monkeypatch):
    """tf_ffn_fused_f32: [LN](x + relu(x w1^T + b1) w2^T + b2) against float64 of the whole block with the hidden layer rounded to fp32:
    the hidden layer's own bound is carried through |w2| into the floor of the output."""
    from trackformer_amd import fused
    M = _ffn_rows_tail() if M == "tail" else M
    monkeypatch.setattr(fused, "_FFN_FUSED_MIN_ROWS", 1)
    x, w1, b1, _ = U.linear_operands(profile, M, D, Fd, seed=M + Fd + ti, device=dev)
    _, w2, b2, _ = U.linear_operands("unit" if profile in ("large_x", "small_x", "row_spread", "nonfinite") else profile, 4, Fd, D,
                                     seed=M + Fd + ti + 1, device=dev)
    gamma, beta = _norm(D, dev, ti)
    l1, l2, norm = _module(w1, b1), _module(w2, b2), torch.nn.LayerNorm(D).to(dev)
    with torch.no_grad():
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    prev_on, prev_ti, prev_tail = fused.set_ffn_fused(True), _option("ffn_ti", ti), _option("ffn_tail_split", 1)
    try:
        with torch.no_grad():
            y = fused.ffn(x, l1, l2, norm if ln else None, residual=x)
    finally:
        fused.set_ffn_fused(prev_on)
        _option("ffn_ti", prev_ti)
        _option("ffn_tail_split", prev_tail)
    assert y is not None
    h, S1, floor1, nan1 = U.linear_reference(x, w1, b1, relu=True, terms=terms)
    # rows whose hidden layer comes within 2 % of the fp16 scheme's limit may or may not overflow: left out
    hmax = torch.where(nan1, torch.zeros_like(h), h.abs()).amax(1)
    unsure = (hmax > 0.98 * U.F16_ACTIVATION_LIMIT) & (hmax < 1.02 * U.F16_ACTIVATION_LIMIT) if terms == 16 else torch.zeros_like(hmax, dtype=torch.bool)
    h32 = torch.where(nan1, h, h.float().double())
    e1 = torch.where(nan1, torch.zeros_like(h), floor1 + U.BOUND * S1)
    pre, S2, floor2, nan2 = U.linear_reference(h32, w2, b2, x, terms=terms)
    nan = nan2 | nan1.any(1, keepdim=True)
    floor = floor2 + e1 @ w2.double().abs().t()
    keep = ~unsure
    if ln:
        _check_ln("ffn_fused_ln", terms, profile, y, pre, S2, floor, nan, gamma, beta, 1e-5, keep=keep)
    else:
        worst = U.check(y[keep], pre[keep], S2[keep], floor[keep], nan[keep])
        _report("ffn_fused", terms, profile, worst)


# ---- convolutions ----------------------------------------------------------------------------------------------------------------------
def _check_conv(entry, terms, profile, y_nhwc, x, wt, b, stride, padding, relu, rows=None):
    ref, S, floor, nan = U.conv_reference(x, wt, b, stride, padding, relu, terms, rows=rows)
    y2 = y_nhwc.reshape(-1, wt.shape[0])
    if rows is not None:
        y2 = y2[rows.to(y2.device)]
    worst = U.check(y2, ref, S, floor, nan, fp32=U.conv_fp32(x, wt, b, stride, padding, relu, rows=rows), k=wt[0].numel())
    _report(entry, terms, profile, worst)


CONV = [  # n, h, w, cin, cout, ks, stride, ksplit
    (1, 1, 1, 64, 64, 3, 1, 1), (2, 2, 1, 64, 96, 3, 1, 1), (1, 9, 7, 64, 128, 3, 2, 1), (1, 11, 13, 64, 160, 3, 1, 5),
    (1, 7, 9, 128, 64, 1, 2, 1), (1, 5, 3, 256, 64, 1, 1, 3)]


def _taps(wt):
    cout, cin, k, _ = wt.shape
    return wt.permute(0, 2, 3, 1).reshape(cout, k * k * cin).contiguous()


CONV_PACKED = [c + (False,) for c in CONV] + [c + (True,) for c in CONV if c[5] == 3 and c[6] == 1]   # + the halo form (stride-1 3 x 3)


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("n,h,w,cin,cout,ks,stride,ksplit,halo", CONV_PACKED,
                         ids=["%dx%dx%d_%d-%d_k%d_s%d_p%d_%s" % (s[:8] + ("halo" if s[8] else "stream",)) for s in CONV_PACKED])
def test_conv_packed(dev, terms, profile, n, h, w, cin, cout, ks, stride, ksplit, halo):
    """tf_conv_packed_f32: tap-major 3 x 3 (stream and halo form), 1 x 1 (strided), split-K pieces (+ the reduce), bias + ReLU."""
    from trackformer_amd import _cabi, fused
    x, wt, b = U.conv_operands(profile, n, cin, h, w, cout, ks, seed=n + h + w + cin + cout, device=dev)
    taps = _taps(wt)
    pad = 1 if ks == 3 else 0
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    prev = fused.set_conv_halo(halo)
    try:
        packed = fused._packed_weight(taps, None)
        y = torch.full((n, ho, wo, cout), float("nan"), device=dev)
        ws = torch.empty((ksplit, n * ho * wo * cout), device=dev) if ksplit > 1 else None
        rc = _cabi.lib().tf_conv_packed_f32(x.data_ptr(), packed.data_ptr(), b.data_ptr(), 0, y.data_ptr(), fused._ptr(ws), ksplit,
                                            n, h, w, cin, cout, ks, stride, 1, terms, fused._stream(dev))
        _cabi.check(rc, "tf_conv_packed_f32")
    finally:
        fused.set_conv_halo(prev)
    _check_conv("conv_packed_halo" if halo else "conv_packed", terms, profile, y, x, wt, b, stride, pad, True)


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("n,h,w,cin,cout,ks,stride,ksplit", CONV, ids=["%dx%dx%d_%d-%d_k%d_s%d_p%d" % s for s in CONV])
def test_conv_block_kernels(dev, terms, profile, n, h, w, cin, cout, ks, stride, ksplit):
    """tf_conv3x3_split_f32 / _splitk_f32, tf_conv1x1_strided_split_f32 / tf_conv1x1_splitk_f32 (the LDS-staged block kernels)."""
    from trackformer_amd import _cabi, fused
    x, wt, b = U.conv_operands(profile, n, cin, h, w, cout, ks, seed=n + h + w + cin + cout + 1, device=dev)
    taps = _taps(wt)
    pad = 1 if ks == 3 else 0
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    hi, mid, lo, wsc = fused._split_weight(taps)
    y = torch.full((n, ho, wo, cout), float("nan"), device=dev)
    L = _cabi.lib()
    if ksplit > 1:
        ws = torch.empty((ksplit, n * ho * wo * cout), device=dev)
        fn = L.tf_conv3x3_splitk_f32 if ks == 3 else L.tf_conv1x1_splitk_f32
        rc = fn(x.data_ptr(), hi.data_ptr(), mid.data_ptr(), fused._ptr(lo), fused._ptr(wsc), b.data_ptr(), y.data_ptr(), ws.data_ptr(),
                ksplit, n, h, w, cin, cout, stride, 1, fused._stream(dev))
    else:
        fn = L.tf_conv3x3_split_f32 if ks == 3 else L.tf_conv1x1_strided_split_f32
        rc = fn(x.data_ptr(), hi.data_ptr(), mid.data_ptr(), fused._ptr(lo), fused._ptr(wsc), b.data_ptr(), y.data_ptr(),
                n, h, w, cin, cout, stride, 1, fused._stream(dev))
    _cabi.check(rc, "conv block kernel")
    _check_conv("conv_block" if ksplit == 1 else "conv_block_splitk", terms, profile, y, x, wt, b, stride, pad, True)


STEM = [(1, 1, 1), (1, 9, 7), (2, 97, 130), (1, 800, 1333)]


@pytest.mark.parametrize("profile", PROFILES)
@pytest.mark.parametrize("n,h,w", STEM, ids=["%dx%dx%d" % s for s in STEM])
def test_stem_conv(dev, terms, profile, n, h, w):
    """tf_stem_conv7x7_f32 with and without shift + ReLU; the full-size frame on 4096 sampled output pixels."""
    from trackformer_amd import fused
    x, wt, b = U.conv_operands(profile, n, 3, h, w, 64, 7, seed=n + h + w, device=dev)
    x = x.contiguous()
    prev = fused.set_stem_conv_split(True)
    try:
        y = fused.stem_conv(x, wt)
        yb = fused.stem_conv(x, wt, b, relu=True)
    finally:
        fused.set_stem_conv_split(prev)
    assert y is not None and y.is_contiguous(memory_format=torch.channels_last)
    m = y.shape[0] * y.shape[2] * y.shape[3]
    rows = None
    if m > 20000:
        rows = torch.randperm(m, generator=torch.Generator().manual_seed(h))[:4096]
        rows[:2] = torch.tensor([0, m - 1])
    _check_conv("stem", terms, profile, y.permute(0, 2, 3, 1), x, wt, None, 2, 3, False, rows)
    _check_conv("stem_relu", terms, profile, yb.permute(0, 2, 3, 1), x, wt, b, 2, 3, True, rows)


@pytest.mark.parametrize("profile", PROFILES)
def test_conv3x3_merge_packed(dev, terms, profile):
    """tf_conv3x3_merge_packed_f32 at the mask head's shapes (lay2: 288 -> 128 channels, two queries per image): the convolution of
    the nearest up-sampled low + fpn, against float64 of the merged input; S from |up(low)| + |fpn|."""
    from trackformer_amd import fused
    n, qpi, (lh, lw), (H, W), cin, cout = 4, 2, (3, 5), (6, 10), 288, 128
    low, wt, b = U.conv_operands(profile, n, cin, lh, lw, cout, 3, seed=7, device=dev)
    fpn, _, _ = U.conv_operands("unit" if profile in ("nonfinite", "large_x") else profile, n // qpi, cin, H, W, cout, 3, seed=8, device=dev)
    prev = fused.set_conv_halo(True)
    try:
        y = fused.conv3x3_merged(low, fpn, qpi, _taps(wt), b)
    finally:
        fused.set_conv_halo(prev)
    assert y is not None
    up = F.interpolate(low.double(), size=(H, W), mode="nearest")
    fb = fpn.double().repeat_interleave(qpi, 0)
    ref, _, _, nan = U.conv_reference(up + fb, wt, b, 1, 1, False, terms)
    _, S, _, _ = U.conv_reference(up.abs() + fb.abs(), wt, b, 1, 1, False, terms)
    merged32 = (up.float() + fb.float())
    _, _, floor, _ = U.conv_reference(merged32, wt, b, 1, 1, False, terms)
    worst = U.check(y.permute(0, 2, 3, 1).reshape(-1, cout), ref, S, floor, nan, fp32=U.conv_fp32(merged32, wt, b, 1, 1), k=9 * cin)
    _report("conv3x3_merge", terms, profile, worst)


# ---- the test of the test --------------------------------------------------------------------------------------------------------------
def test_yardstick_rejects_a_product_without_the_lower_weight_piece(dev):
    """tf_linear_split_f32 of the fp16 scheme with the lower weight piece replaced by zeros (pieces passed straight to the C ABI):
    the hardware result carries the hi piece's 2^-12 relative error and the yardstick must reject it, while the same call with the
    true pieces passes."""
    from trackformer_amd import _cabi, fused
    prev = fused.set_split_terms(16)
    try:
        M, K, N = 300, 256, 192
        x, w, b, _ = U.linear_operands("unit", M, K, N, seed=3, device=dev)
        wh, wl, _, sc = fused._split_weight(w)
        outs = []
        for lo in (wl, torch.zeros_like(wl)):
            y = torch.empty((M, N), device=dev)
            rc = _cabi.lib().tf_linear_split_f32(x.data_ptr(), wh.data_ptr(), lo.data_ptr(), 0, sc.data_ptr(), b.data_ptr(), y.data_ptr(),
                                                 M, K, N, 0, fused._stream(dev))
            _cabi.check(rc, "tf_linear_split_f32")
            outs.append(y)
    finally:
        fused.set_split_terms(prev)
    ref, S, floor, nan = U.linear_reference(x, w, b, terms=16)
    fp32 = U.linear_fp32(x, w, b)
    U.check(outs[0], ref, S, floor, nan, fp32=fp32)
    with pytest.raises(AssertionError):
        U.check(outs[1], ref, S, floor, nan, fp32=fp32)
