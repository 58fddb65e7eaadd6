"""The float64 yardstick of the split product (trackformer_amd/csrc/split_product.h) and the magnitude profiles every split-product
test draws its operands from.

A split-product result y is held to the float64 result `ref` of the same operation, per output element:

    (|y - ref| - floor) / S  <=  2^-20          S = sum_k |x_mk| |w_nk| + |b_n| + |r_mn|

For a long K (the 3 x 3 convolutions over 288 channels: K = 2592) the fixed bound grows as 2^-20 sqrt(K / 1152): the matrix cores
round their fp32 accumulator once per MFMA along K, and the error of such a sum grows as sqrt(K) (measured on MI355X: 1.0e-6 at K =
2592 under six terms, where torch's fp32 result itself reaches 6.4e-7).

floor: the fp16 scheme (terms = 16) represents an activation below 2^-10 to an ABSOLUTE 2^-32 only (its hi piece is an fp16
subnormal after the 2^-4 activation scaling), so an output may carry 2^-31 sum_k |w_nk| over those k that does not shrink with
the row.  Beside that, both schemes and fp32 itself hold numbers in and near the fp32 subnormals to an absolute spacing only
(small_floor() lists the terms); they matter for outputs of order 1e-38 and nothing else.  Next to that fixed bound the result is held to torch's CPU fp32 result on the
same operands (a plain sgemm; a convolution as sgemm over its unfolded input): its largest excess may be at most four times the
fp32 result's own largest normalised error (2^-21 where the fp32 result is as good as exact: a few outputs, a short K) -- the
matrix cores sum along K one MFMA at a time where a CPU sgemm sums in blocks (measured on MI355X: up to 3.5 x the CPU's worst
element).  A result that is fp32-class passes, one good to "almost" (a single fp16 piece: 2^-11, a single bf16 piece: 2^-8, the
fp16 scheme without its lower weight piece: 2^-12) does not.

Non-finite contract: a NaN activation, or under the fp16 scheme one above fused.F16_ACTIVATION_LIMIT, makes exactly the outputs
that read it NaN (its own row of a linear, the pixels whose window holds it in a convolution); every other output is finite and
within the bound.

Everything here is torch and runs on the CPU or the GPU (float64 there as well)."""
import math

import torch
import torch.nn.functional as F

BOUND = 2.0 ** -20            # the fixed bound on (|y - ref| - floor) / S, for K up to BOUND_K ...
BOUND_K = 1152                # ... beyond it 2^-20 sqrt(K / 1152): fp32 accumulation's rounding grows as sqrt(K)
FP32_FACTOR = 4.0             # the fp32 comparison: at most 4 x the fp32 result's own worst normalised error ...
FP32_CLASS_MIN = 2.0 ** -21   # ... or 2^-21 where the fp32 result itself is as good as exact
SMALL_ACT = 2.0 ** -10        # fp16 scheme: activations below this carry an absolute error ...
FLOOR_PER_W = 2.0 ** -31      # ... of at most 2^-32: the floor is 2^-31 sum |w| over them (a factor 2 of margin)
F16_ACTIVATION_LIMIT = 65504.0 * 16.0   # (= fused.F16_ACTIVATION_LIMIT; asserted by the CPU self-test)

PROFILES = ["unit", "small_x", "large_x", "row_spread", "channel_spread", "edge_values"]
SUBNORMAL = 1e-40


class Excess:
    """The worst element of a comparison: its normalised excess over the floor, where it is, and the values there."""

    def __init__(self, value, index, got, want, scale, floor, fp32_err):
        self.value, self.index, self.got, self.want, self.scale, self.floor, self.fp32_err = value, index, got, want, scale, floor, fp32_err

    def __repr__(self):
        return ("max (|y - ref| - floor) / S = %.3e at %s (y %r, ref %r, S %.3e, floor %.3e); fp32 result's own max error %.3e"
                % (self.value, self.index, self.got, self.want, self.scale, self.floor, self.fp32_err))


def _normalised(err, scale):
    """err / scale with 0 / 0 = 0 and e / 0 = inf (an output whose S is zero must come out exact)."""
    err = err.clamp_min(0)
    return torch.where(scale > 0, err / torch.where(scale > 0, scale, torch.ones_like(scale)),
                       torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


def excess(y, ref, scale, floor=None, expect_nan=None, fp32=None):
    """Normalised excess of y over the floor, per element, and the worst element (Excess).  expect_nan: boolean mask of the outputs
    that must be NaN (checked here: exactly those are NaN, every other output is finite).  fp32: torch's fp32 result of the same
    operation (its own normalised error is reported on the Excess)."""
    y = y.double()
    ref = ref.double()
    scale = scale.double().expand_as(ref)
    floor = torch.zeros_like(ref) if floor is None else floor.double().expand_as(ref)
    if expect_nan is None:
        expect_nan = torch.zeros(ref.shape, dtype=torch.bool, device=ref.device)
    expect_nan = expect_nan.expand_as(ref)
    bad_nan = torch.isnan(y) != expect_nan
    assert not bool(bad_nan.any()), "NaN outputs do not match the expected ones at %s (y %r)" % (
        tuple(int(v) for v in bad_nan.nonzero()[0]), float(y[bad_nan][0]))
    keep = ~expect_nan
    assert bool(torch.isfinite(y[keep]).all()), "non-finite output where none is expected"
    e = torch.where(keep, _normalised((y - ref).abs() - floor, scale), torch.zeros_like(ref))
    flat = int(e.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), e.shape))
    fp32_err = 0.0
    if fp32 is not None:
        f = torch.where(keep, _normalised((fp32.double().to(ref.device) - ref).abs(), scale), torch.zeros_like(ref))
        fp32_err = float(f.max())
    return e, Excess(float(e.reshape(-1)[flat]), idx, float(y[idx]), float(ref[idx]), float(scale[idx]), float(floor[idx]), fp32_err)


def bound_for(k):
    """The fixed bound for a sum over k products."""
    return BOUND * max(1.0, (k / BOUND_K) ** 0.5)


def check(y, ref, scale, floor=None, expect_nan=None, fp32=None, k=None):
    """Assert the yardstick (module docstring) for sums over k products (None: at most BOUND_K) and return the worst element (Excess)."""
    _, worst = excess(y, ref, scale, floor, expect_nan, fp32)
    assert worst.value <= bound_for(k or 0), worst
    if fp32 is not None:
        assert worst.value <= max(FP32_FACTOR * worst.fp32_err, FP32_CLASS_MIN), worst
    return worst


# ---- references ----------------------------------------------------------------------------------------------------------------------
def small_floor(x2, w2, terms):
    """The absolute floor per output of x2 [M, K] . w2 [N, K]^T (module docstring):
      both schemes   2^-149 (K + 2): fp32 arithmetic itself, whose spacing in the subnormals is 2^-149 (products and sums)
      terms = 16     + 2^-31 sum_{k: |x_mk| < 2^-10} |w_nk|: activations below 2^-10 are held to an absolute 2^-32
                     + 2^-150 sum_k |x_mk|: a channel whose largest |w| lies below 2^-112 (the weight scale's cap, split_product.h)
      terms = 6      + 2^-133 (sum_{k: |x_mk| < 2^-109} |w_nk| + sum_{k: |w_nk| < 2^-109} |x_mk|): three bf16 pieces hold a number to
                     an absolute 2^-134 (bf16's subnormal spacing is 2^-133), i.e. to all 24 bits only above 2^-110"""
    K = x2.shape[1]
    xa, wa = x2.double().abs(), w2.double().abs()
    floor = torch.full((x2.shape[0], w2.shape[0]), 2.0 ** -149 * (K + 2), dtype=torch.float64, device=x2.device)
    if terms == 16:
        floor = floor + FLOOR_PER_W * ((xa < SMALL_ACT).double() @ wa.t()) + 2.0 ** -150 * xa.sum(1, keepdim=True)
    else:
        tiny = 2.0 ** -109
        floor = floor + 2.0 ** -133 * ((xa < tiny).double() @ wa.t() + xa @ (wa < tiny).double().t())
    return floor


def over_limit(x, terms):
    """Activations the fp16 scheme cannot represent (NaN included; under six terms: NaN only)."""
    bad = torch.isnan(x)
    if terms == 16:
        bad = bad | ~(x.abs() < F16_ACTIVATION_LIMIT)
    return bad


def linear_reference(x, w, b=None, residual=None, relu=False, terms=16):
    """act(x w^T + b + residual) in float64 for x [M, K], w [N, K] -> (ref, S, floor, expect_nan) for check()."""
    xd, wd = x.double(), w.double()
    pre = xd @ wd.t()
    scale = xd.abs() @ wd.abs().t()
    if b is not None:
        pre = pre + b.double()
        scale = scale + b.double().abs()
    if residual is not None:
        pre = pre + residual.double()
        scale = scale + residual.double().abs()
    ref = pre.clamp_min(0) if relu else pre
    expect_nan = over_limit(x, terms).any(1, keepdim=True).expand_as(ref) | torch.isnan(ref)
    return ref, scale, small_floor(x, w, terms), expect_nan


def linear_fp32(x, w, b=None, residual=None, relu=False):
    """torch's fp32 result of the same linear, on the CPU."""
    y = x.float().cpu() @ w.float().cpu().t()
    if b is not None:
        y = y + b.float().cpu()
    if residual is not None:
        y = y + residual.float().cpu()
    return y.clamp_min(0) if relu else y


def _unfold(x_nchw, kh, kw, stride, padding):
    """[N, C, H, W] -> [N * Ho * Wo, C * kh * kw] (rows in NHWC order of the output, columns in [C, kh, kw] order)."""
    n, c, h, w = x_nchw.shape
    ho, wo = (h + 2 * padding - kh) // stride + 1, (w + 2 * padding - kw) // stride + 1
    cols = F.unfold(x_nchw, (kh, kw), padding=padding, stride=stride)        # [N, C kh kw, Ho Wo]
    return cols.transpose(1, 2).reshape(n * ho * wo, c * kh * kw), (n, ho, wo)


def conv_reference(x, w, b=None, stride=1, padding=0, relu=False, terms=16, residual=None, rows=None):
    """A convolution in float64 for x [N, Cin, H, W] (NCHW or channels_last storage) and w [Cout, Cin, kh, kw] -> (ref, S, floor,
    expect_nan) for check(), all [N * Ho * Wo, Cout] in NHWC order of the output (the storage of a channels_last result); S and
    the floor are the float64 convolutions of |x| and |w| (and of the small-activation indicator).  residual: [N * Ho * Wo, Cout].
    rows: output pixels to compute (a LongTensor index into the N * Ho * Wo rows; the full-size shapes compare a sample)."""
    cout, cin, kh, kw = w.shape
    cols, _ = _unfold(x.double(), kh, kw, stride, padding)
    if rows is not None:
        cols = cols[rows.to(cols.device)]
    w2 = w.double().reshape(cout, cin * kh * kw)
    return linear_reference(cols, w2, b, residual, relu, terms)   # (a window holding a bad activation: its row of `cols`)


def conv_fp32(x, w, b=None, stride=1, padding=0, relu=False, residual=None, rows=None):
    """torch's fp32 convolution result on the CPU in the layout of conv_reference()."""
    cout, cin, kh, kw = w.shape
    cols, _ = _unfold(x.float().cpu(), kh, kw, stride, padding)   # (an sgemm: torch's CPU convolution may take another algorithm)
    if rows is not None:
        cols = cols[rows.cpu()]
    return linear_fp32(cols, w.reshape(cout, cin * kh * kw), b, residual, relu)


def layernorm_reference(pre, scale, floor, gamma, beta, eps, expect_nan, bound=BOUND):
    """float64 LayerNorm over the last dimension of the pre-norm sum `pre` [M, D], with the norm-aware bound: the pre-norm bound
    e_i = floor_i + bound S_i moves z_i = (p_i - mean) / std by at most (e_i + max_j e_j) / std (the mean and the variance take
    their share of every e_j), and fp32 LayerNorm arithmetic adds a few ulp of (|mean| + |p|) / std -> (ref, S', floor') for
    check() with S' = |gamma| (max_j |p_j| + |p_i| + |mean|) / std + |beta| + |gamma z_i| and floor' = |gamma| (e_i + max_j e_j) / std."""
    mean = pre.mean(-1, keepdim=True)
    var = pre.var(-1, unbiased=False, keepdim=True)
    std = (var + eps).sqrt()
    z = (pre - mean) / std
    g, be = gamma.double(), beta.double()
    ref = z * g + be
    e = floor + bound * scale
    e = torch.where(expect_nan, torch.zeros_like(e), e)
    emax = e.amax(-1, keepdim=True)
    floor_n = g.abs() * (e + emax) / std
    scale_n = g.abs() * (pre.abs().amax(-1, keepdim=True) + pre.abs() + mean.abs()) / std + be.abs() + (g * z).abs()
    return ref, scale_n, floor_n, expect_nan.any(-1, keepdim=True).expand_as(ref)


# ---- magnitude profiles ----------------------------------------------------------------------------------------------------------------
def shape_activations(x2, profile, generator=None):
    """Apply `profile` in place to the rows [M, K] of an activation (for a convolution: the channels_last pixels [N H W, Cin])."""
    M, K = x2.shape
    if profile == "small_x":
        x2.mul_(1e-4)
    elif profile == "large_x":
        x2.mul_(300.0)
        r = M // 2
        x2[r] *= 0.9 * F16_ACTIVATION_LIMIT / float(x2[r].abs().max())
    elif profile == "row_spread":
        x2[::5] *= 1e-2
        x2[2::9] *= 1e2
    elif profile == "edge_values":
        sign = torch.where(x2 < 0, -1.0, 1.0)
        x2[::7, ::3] = sign[::7, ::3] * SUBNORMAL              # scattered fp32 subnormals
        if M > 1:
            x2[1] = sign[1] * SUBNORMAL                       # a row of them
        x2[::4, 1::5] = -0.0
        if M > 3:
            x2[3] = 0.0                                       # an all-zero row
    elif profile not in ("unit", "channel_spread"):
        raise ValueError(profile)
    return x2


def shape_weights(w2, profile):
    """Apply `profile` in place to a weight [N, K] (for a convolution: [Cout, kh kw Cin] or [Cout, Cin kh kw], any order of K)."""
    N = w2.shape[0]
    if profile == "channel_spread":
        w2[::7] *= 1e-3          # FrozenBN folded into a convolution: channels of very different scale
        w2[3::11] *= 100.0
    elif profile == "edge_values":
        w2[0] = 0.0              # the amax == 0 branch of the per-channel weight scale
        if N > 1:
            w2[N - 1] = torch.where(w2[N - 1] < 0, -SUBNORMAL, SUBNORMAL)   # a channel of fp32 subnormals
        w2[:, ::6] *= 0.0        # signed zeros
    return w2


def add_nonfinite(x2, rows):
    """The non-finite contract's operands: a NaN in row rows[0], one activation beyond the fp16 scheme's limit in row rows[1]."""
    K = x2.shape[1]
    x2[rows[0], K // 3] = float("nan")
    if len(rows) > 1:
        x2[rows[1], (2 * K) // 3] = 2.0 * F16_ACTIVATION_LIMIT
    return x2


def linear_operands(profile, M, K, N, seed, device="cpu", bias=True, residual=False):
    """Seeded (x [M, K], w [N, K], b [N] or None, r [M, N] or None) for `profile` ("nonfinite": unit operands plus add_nonfinite)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if bias else None
    r = torch.randn(M, N, generator=g) if residual else None
    if profile == "nonfinite":
        add_nonfinite(x, [M // 3, (2 * M) // 3] if M > 2 else [0])
    else:
        shape_activations(x, profile, g)
        shape_weights(w, profile)
    return tuple(None if t is None else t.to(device) for t in (x, w, b, r))


def conv_operands(profile, n, cin, h, w, cout, k, seed, device="cpu", bias=True):
    """Seeded channels_last x [n, cin, h, w], weight [cout, cin, k, k], bias [cout] or None for `profile`."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, cin, generator=g)                      # NHWC storage: the pixel rows are x.view(-1, cin)
    wt = torch.randn(cout, cin, k, k, generator=g) / (k * cin ** 0.5)
    b = torch.randn(cout, generator=g) if bias else None
    x2 = x.view(-1, cin)
    if profile == "nonfinite":
        m = x2.shape[0]
        add_nonfinite(x2, [m // 3, (2 * m) // 3] if m > 2 else [0])
    else:
        shape_activations(x2, profile, g)
        shape_weights(wt.view(cout, -1), profile)
    x = x.permute(0, 3, 1, 2)                                           # NCHW shape over NHWC storage
    return x.to(device), wt.to(device), None if b is None else b.to(device)

