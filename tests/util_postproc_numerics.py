"""The float64 yardsticks of the post-processing and pooling kernels of trackformer_amd/csrc/fused_ops.hip -- the kernels whose outputs
are DECISIONS or INDICES rather than sums (tf_mask_label_map_f32, tf_postprocess_pack_f32) or exactly selected operands added once or
twice (tf_bias_relu_maxpool_f32, tf_upsample_add_nhwc_f32, tf_bias_act_f32) -- the operand profiles and size tables every numerics
test of them draws from, and fp32 numpy models of the documented operations with named MUTANTS (the CPU self-test proves that the
rules below reject each of them).  Nothing here comes from the code under test: every formula is the published definition of the
torch operation the kernel replaces.

Index arithmetic is part of the contract and is restated exactly, in numpy.float32, one rounding per operation:

    nearest (torch's legacy "nearest"):        src = min(int(floorf(dst * ((float)in / (float)out))), in - 1)
    bilinear, align_corners = False:           s = max(((float)in / (float)out) * (dst + 0.5f) - 0.5f, 0),  i0 = (int)s,
                                               i1 = i0 + (i0 < in - 1),  l1 = s - i0,  l0 = 1 - l1

selftest_index_arithmetic() holds both against torch.nn.functional.interpolate on the CPU over every pair in < 40, out < 90; the fp32
nearest index differs from the exact integer dst * in // out at, e.g., (in, out) = (2, 82), (4, 82), (6, 74), (8, 82), and the size
tables below contain such pairs (FP32_VS_EXACT_PAIRS), so an "exact" integer re-implementation of the index fails.

Values are float64: with the exact indices and the fp32 weights widened to double, v = l0y (l0x a + l1x b) + l1y (l0x c + l1x d),
Sv = the same sum over |.|, p = sigmoid(v).

THE DECISION RULE (label-map owner, post-process label, threshold).  An fp32 probability is within

    tol = c (1 + Sv),   c = C_TOL = 2^-22

of the float64 one.  Derivation (u = 2^-24): every term of the bilinear form passes two multiplies and two adds (one multiply and one
add per level), so |v32 - v| <= ((1 + u)^4 - 1) Sv ~ 4 u Sv, and sigmoid' <= 1/4 carries that into the probability as u Sv.  The
sigmoid itself: expf with a relative error of up to 2 ulp = 4 u reaches p = 1 / (1 + e) as p (1 - p) 4 u <= u; the addition and the
division add u p each.  |p32 - p64| <= u Sv + 3 u <= 3 u (1 + Sv), rounded up to the next power of two (which also covers the second-
order terms): 4 u = 2^-22.  (For the post-process score Sv = |logit|; the logit is exact there, so the bound has room.)  Where v is
+-inf the probability is exactly 0 or 1 in either precision and tol = 0.

  * a track (class) t is ACCEPTABLE for a pixel (query) when p64[t] + tol[t] >= max_s (p64[s] - tol[s]): the kernel's answer is the
    maximum of ITS probabilities, so it can only be such a t.  The answer must be acceptable.  (The issue that asked for this rule worded
    the set one-sidedly, p64[t] >= max p64 - tol with a trial c = 2^-21.  Both probabilities of a comparison carry an error, each with
    its own Sv, so the two-sided form is the sound one; with c = 2^-22 on either side the total margin is that trial's.)
  * if max_s (p64[s] - tol[s]) > thr the answer must not be -1; if max_s (p64[s] + tol[s]) < thr it must be -1;
  * a track whose logits are bitwise those of an earlier track in `order` (the same row twice, or two equal rows) is never
    acceptable: the update is a strict `>`, the first of them wins on every pixel;
  * a pixel whose probabilities hold a NaN is -1 (`stack -> max -> best > thr`: torch.max returns the NaN);
  * a pixel is AMBIGUOUS when thr lies inside [max (p - tol), max (p + tol)], or when more than one track is acceptable and the pixel is
    not -1 whichever of them wins (max (p + tol) < thr).  Every other pixel therefore equals the float64 decision exactly.  No share of pixels is excused.
  * so that the rule cannot go vacuous, the ambiguous share of every (profile, shape) that takes part in it is capped at AMBIG_CAP =
    1e-2, asserted on the float64 reference alone before a kernel is looked at.

Saturation and exact ties get exact tests instead of a margin: bitwise equal rows, rows with every logit >= 40 (all probabilities
exactly 1.0f), subnormal logits (every probability exactly 0.5f) and all-zero logits (0.5 is not > 0.5: the map is all -1, which is
what rejects a `>=` at the threshold) go to the first track / class in order, on every pixel.

Measured worst |p32 - p64| / tol on the CPU (test_postproc_numerics_cpu.py, every profile, Q up to 100000): torch's fp32
sigmoid().max(-1) 0.242, the emulated post-process kernel 0.239; the emulated label map has no pixel outside the rule and no pixel off
the float64 decision that is not ambiguous.  First MI355X figures (the device's expf; `pytest -s
tests/test_postproc_numerics_gpu.py` prints them per case, profiles/postproc_numerics_gpu_first_run.txt keeps them): the post-process
kernel's worst |s - p64| / tol 0.251, torch's fp32 chain on the device 0.251 on the same logits; at most 6 labels per case off the float64
argmax, all ambiguous, none off the chain on the device (largest ambiguous share of a margin profile 5.0e-3); boxes bit-equal to the
numpy.float32 restatement and to the chain on the device.  Label map, 196 (profile, shape, order) cases: 0 violations, largest
ambiguous share 2.5e-3, at most 81 pixels of a map (1060 in all) off the float64 decision, every one of them ambiguous.  c was not
fitted to any of this.

Values that are not decisions
  * post-process boxes: every operation is one correctly rounded fp32 operation (contraction off), so the numpy.float32 restatement
    must match bit for bit; they are also held to float64 within 2 ulp (2^-22) of max(|coordinate|, image side), so that a
    restatement that shares a mistake with the kernel is still caught.  Scores: |s - p64| <= tol, and the worst |s - p64| / (1 +
    |logit|) at most 4 x torch's fp32 sigmoid's on the same logits, or 2^-23.
  * tf_upsample_add_nhwc_f32, tf_bias_act_f32, tf_bias_relu_maxpool_f32: one or two fp32 additions of exactly selected operands.  The
    float64 result rounded ONCE (bias_act with a residual: rounded after each of its two additions, in the documented order (x + bias)
    + residual) must equal the output bit for bit, NaN positions included (NaN payloads are not compared).  This is stricter than a
    bound and is what the kernels claim.  ReLU is `v < 0 ? 0 : v`: it keeps -0.0 and NaN, as torch's relu on the CPU does.  torch's relu
    on MI355X does NOT: relu(-0.0) and clamp_min(-0.0, 0) give +0.0 there (max_pool2d keeps -0.0 on both).  The kernels are pinned to the
    CPU behaviour they have today (the reference above); against the chain on the device the `signed_zero` profile compares values and
    reports the zeros whose sign differs (against_device_chain()), every other profile compares every bit.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
C_TOL = 2.0 ** -22
AMBIG_CAP = 1e-2
FP32_FACTOR = 4.0
FP32_CLASS_MIN = 2.0 ** -23
BOX_ULPS = 2.0 ** -22

f32 = np.float32

# (in, out) pairs at which the fp32 nearest index differs from dst * in // out somewhere
FP32_VS_EXACT_PAIRS = [(2, 82), (4, 82), (6, 74), (8, 82)]

LABEL_PROFILES = ["unit", "flat", "peaked", "threshold", "threshold03", "large", "neg"]       # take part in the margin rule
ADD_PROFILES = ["unit", "large", "cancel", "signed_zero", "non_finite"]
POST_PROFILES = ["unit", "flat", "peaked", "large", "neg"]

# label-map cases: (h, w) logits, pad, img, out, tracks.  CPU: what the emulator finishes quickly; GPU: the model's geometry and edges
LABEL_CASES_CPU = [
    ((13, 21), (50, 84), (50, 84), (67, 107), 7),
    ((25, 42), (100, 168), (91, 160), (67, 107), 7),        # crop in both directions, out < img
    ((13, 21), (52, 84), (50, 84), (50, 84), 20),           # crop in one direction, out == img
    ((6, 8), (24, 32), (6, 8), (74, 82), 5),                # nearest 6 -> 74, 8 -> 82: fp32 index != exact index
    ((1, 9), (4, 36), (4, 33), (9, 70), 3),                 # h == 1
    ((7, 1), (28, 4), (28, 4), (31, 5), 3),                 # w == 1, out smaller than one 32 x 8 tile
    ((1, 1), (4, 4), (2, 2), (3, 3), 2),
]
LABEL_CASES_GPU = LABEL_CASES_CPU + [
    ((200, 334), (800, 1333), (800, 1333), (1080, 1920), 1),
    ((200, 334), (800, 1333), (800, 1333), (1080, 1800), 7),
    ((200, 334), (800, 1333), (800, 1333), (1080, 1920), 100),
    ((200, 334), (800, 1344), (800, 1333), (1080, 1800), 100),
    ((200, 334), (800, 1333), (800, 1333), (1080, 1800), 400),
    ((50, 84), (200, 336), (187, 333), (270, 450), 20),
    ((50, 84), (200, 336), (200, 336), (100, 168), 20),     # out < img
    ((13, 21), (50, 84), (50, 84), (50, 84), 100),
    ((4, 2), (82, 82), (4, 2), (82, 82), 4),                # nearest 4 -> 82, 2 -> 82
]
POST_Q = [1, 255, 256, 257, 300, 400, 100000]
POST_C = [1, 2, 20, 91]
POST_SIDES = [(1080, 1920), (375, 1242), (1, 1)]
POOL_SHAPES_CPU = [(1, 20, 33, 64), (2, 7, 8, 8), (1, 1, 1, 4), (1, 2, 5, 12), (3, 1, 6, 4), (2, 9, 2, 8)]                 # N, H, W, C
POOL_SHAPES_GPU = POOL_SHAPES_CPU + [(1, 400, 667, 64), (2, 33, 20, 256), (2, 50, 50, 4), (1, 2, 2, 8), (1, 5, 1, 8)]
# upsample + add: N, q_per_image, (h, w), (H, W), C
UPS_CASES_CPU = [(3, 3, (5, 7), (10, 14), 8), (2, 1, (6, 8), (74, 82), 4), (2, 2, (4, 2), (82, 82), 4), (2, 1, (10, 14), (5, 7), 4),
                 (1, 1, (3, 4), (3, 4), 8), (2, 1, (1, 5), (4, 1), 4), (1, 1, (1, 1), (1, 1), 4)]
UPS_CASES_GPU = UPS_CASES_CPU + [(6, 3, (25, 42), (50, 84), 128), (4, 4, (50, 84), (100, 167), 64), (2, 1, (100, 167), (200, 334), 32),
                                 (100, 100, (13, 21), (25, 42), 8), (4, 1, (100, 167), (200, 334), 128)]   # the last: 8.5 M quads > 8192 x 256
# bias_act: (positions, C): n4 = positions * C / 4 quads
BIAS_ACT_CASES_CPU = [(1, 4), (3, 8), (5, 12), (301, 4), (257, 256), (7, 288), (100, 8)]
BIAS_ACT_CASES_GPU = BIAS_ACT_CASES_CPU + [(4096 * 256 + 37, 4),      # one pass and 37 quads: `two` true for 37 threads, false for the rest
                                            (2 * 4096 * 256 + 1000, 4),   # a second loop trip
                                            (4096 * 64 * 8 + 5, 8), (4096 * 256 // 3 * 2 + 11, 12), (33000, 256), (29131, 288)]


# ---- index arithmetic ------------------------------------------------------------------------------------------------------------
def nearest_index(n_out, n_in, exact=False):
    d = np.arange(n_out)
    if exact:
        return d * n_in // n_out
    scale = f32(n_in) / f32(n_out)
    return np.minimum(np.floor(d.astype(f32) * scale).astype(np.int64), n_in - 1)


def bilinear_taps(dst, n_in, n_out, align_corners=False, clamp=True):
    """dst: integer destination indices in a grid of n_out -> (i0, step to the second tap (0 | 1), l0, l1) in a source of n_in; fp32."""
    dst = np.asarray(dst).astype(f32)
    if align_corners:
        s = (f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)) * dst
    else:
        s = np.maximum(f32(n_in) / f32(n_out) * (dst + f32(0.5)) - f32(0.5), f32(0))
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    step = (i0 < n_in - 1).astype(np.int64) if clamp else np.ones_like(i0)
    l1 = s - i0.astype(f32)
    return i0, step, f32(1) - l1, l1


class Geometry:
    """Per output row / column of the label map: the source taps and weights (module docstring).  `mutant` names a wrong variant."""

    def __init__(self, h, w, pad, img, out, mutant=None):
        exact = mutant == "exact_nearest"
        py, px = nearest_index(out[0], img[0], exact), nearest_index(out[1], img[1], exact)
        gy, gx = pad, pad
        if mutant == "pad_is_img":
            gy = gx = img
        if mutant == "skip_nearest":
            py, px, gy, gx = np.arange(out[0]), np.arange(out[1]), out, out
        ac, clamp = mutant == "align_corners", mutant != "no_clamp"
        self.y0, self.yp, self.ly0, self.ly1 = bilinear_taps(py, h, gy[0], ac, clamp)
        self.x0, self.xp, self.lx0, self.lx1 = bilinear_taps(px, w, gx[1], ac, clamp)
        self.h, self.w, self.out = h, w, tuple(out)


def selftest_index_arithmetic(max_in=40, max_out=90):
    """The numpy.float32 index formulas against torch.nn.functional.interpolate on the CPU, every pair in < max_in, out < max_out;
    returns the pairs whose fp32 nearest index differs from the exact integer one."""
    import torch.nn.functional as F
    differ = []
    for n_in in range(1, max_in):
        ramp = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
        for n_out in range(1, max_out):
            near = F.interpolate(ramp, size=(n_out, 1), mode="nearest").view(-1).numpy().astype(np.int64)
            mine = nearest_index(n_out, n_in)
            assert np.array_equal(near, mine), ("nearest", n_in, n_out)
            if not np.array_equal(mine, nearest_index(n_out, n_in, exact=True)):
                differ.append((n_in, n_out))
            # bilinear of the ramp x -> x is the source coordinate itself: l0 i0 + l1 (i0 + 1) = s (up to an ulp of s)
            lin = F.interpolate(ramp, size=(n_out, 1), mode="bilinear", align_corners=False).view(-1).numpy().astype(np.float64)
            i0, step, l0, l1 = bilinear_taps(np.arange(n_out), n_in, n_out)
            s = l0.astype(np.float64) * i0 + l1.astype(np.float64) * (i0 + step)
            assert np.all(np.abs(lin - s) <= 2.0 ** -22 * np.maximum(s, 1.0)), ("bilinear", n_in, n_out)
    return differ


# ---- operand profiles ------------------------------------------------------------------------------------------------------------
def logit_of(thr):
    return math.log(thr / (1.0 - thr))


def _blocks(rng, h, w, size, high):
    """A block-constant integer field: one draw from [0, high) per size x size block."""
    by, bx = (h + size - 1) // size, (w + size - 1) // size
    return np.repeat(np.repeat(rng.integers(0, high, (by, bx)), size, 0), size, 1)[:h, :w]


def label_logits(profile, n, h, w, seed=0):
    """[n, h, w] fp32 mask logits of a profile (module docstring / LABEL_PROFILES, + the exact-test profiles)."""
    rng = np.random.default_rng(seed * 1000003 + n * 131 + h * 17 + w)
    z = rng.standard_normal((n, h, w))
    if profile == "unit":
        x = z * 3
    elif profile == "flat":
        x = z * 0.01
    elif profile == "peaked":
        # one strong owner per 10 x 10 block over moderate others; the base spread shrinks with the number of tracks so that the two
        # best of them stay apart (ambiguous share against the cap: test_postproc_numerics_cpu.py)
        x = z * (3.0 if n <= 100 else 1.0)
        owner = _blocks(rng, h, w, 10, n)
        boost = np.array([6.0, 9.0, 12.0])[_blocks(rng, h, w, 10, 3)]
        x += (np.arange(n)[:, None, None] == owner[None]) * boost[None]
    elif profile in ("threshold", "threshold03"):
        # every logit a small multiple (64 .. 180) of the rule's tolerance away from logit(thr): above it for the one owner of a 10 x 10
        # block, below it for everybody else
        thr = 0.5 if profile == "threshold" else 0.3
        l0 = logit_of(thr)
        delta = C_TOL * (1 + abs(l0)) / (thr * (1 - thr))
        owner = _blocks(rng, h, w, 10, n + max(n // 2, 1))      # (an owner >= n: nobody is above the threshold in that block)
        sign = np.where(np.arange(n)[:, None, None] == owner[None], 1.0, -1.0)
        x = l0 + sign * delta * (64 + 8 * (np.arange(n) % 15)[:, None, None] + rng.random((n, h, w)) * 4)
    elif profile == "large":
        # |logit| in [1e3, 1e4]: expf(-v) overflows, probabilities are exactly 0 or 1.  One magnitude field for all tracks, positive
        # for the owner of a 10 x 10 block only: between two blocks one owner's sample is exactly minus the other's
        mag = 1e3 + 9e3 * rng.random((h, w))
        owner = _blocks(rng, h, w, 10, n)
        x = np.where(np.arange(n)[:, None, None] == owner[None], mag[None], -mag[None])
    elif profile == "neg":
        x = -np.abs(z * 3) - 0.01
    elif profile == "subnormal":
        x = z * 1e-40
    elif profile == "zero":
        x = np.zeros((n, h, w))
    elif profile == "saturated":
        x = 40.0 + np.abs(z) * 20
    else:
        raise ValueError(profile)
    return x.astype(f32)


def threshold_of(profile):
    return 0.3 if profile == "threshold03" else 0.5


def post_inputs(profile, Q, C, seed=0):
    """(logits [Q, C], boxes [Q, 4]) fp32: boxes inside and outside [0, 1], zero and negative widths."""
    rng = np.random.default_rng(seed * 7919 + Q * 31 + C)
    z = rng.standard_normal((Q, C))
    if profile == "unit":
        x = z * 3
    elif profile == "flat":
        x = z * 0.01
    elif profile == "peaked":
        x = z * (3.0 if C <= 20 else 1.5)          # (many classes: a lower base spread keeps the two best of the others apart)
        x[np.arange(Q), rng.integers(0, C, Q)] += np.array([6.0, 9.0, 12.0])[rng.integers(0, 3, Q)]
    elif profile == "large":
        x = -(1e3 + 9e3 * rng.random((Q, C)))
        k = rng.integers(0, C, Q)
        x[np.arange(Q), k] = -x[np.arange(Q), k] * (rng.random(Q) < 0.7)
    elif profile == "neg":
        x = -np.abs(z * 3) - 0.01
    elif profile == "subnormal":
        x = z * 1e-40
    elif profile == "saturated":
        x = 40.0 + np.abs(z) * 20
    elif profile == "non_finite":
        # NaN / +inf / -inf in the first and in later classes, several NaN in one query (the first of them is the label)
        x = z * 3
        k = rng.random((Q, C))
        x[k < 0.02] = np.nan
        x[(k >= 0.02) & (k < 0.04)] = np.inf
        x[(k >= 0.04) & (k < 0.06)] = -np.inf
        x[::7, 0] = np.nan
        x[3::7, C - 1] = np.nan
        x[5::11, C // 2] = np.inf
    else:
        raise ValueError(profile)
    boxes = rng.random((Q, 4))
    boxes[: Q // 8, 2:] *= 3                      # overflow the image on every side
    boxes[Q // 8: Q // 6, :2] = boxes[Q // 8: Q // 6, :2] * 3 - 1   # centres outside [0, 1]
    boxes[Q // 6: Q // 5, 2] = 0.0                # zero width
    boxes[Q // 5: Q // 4, 3] *= -1.0              # negative height
    return x.astype(f32), boxes.astype(f32)


def additive_operands(profile, shape, C, seed=0, pool=False):
    """(x [shape], bias [C], residual [shape]) fp32 with the channel in the LAST axis of `shape`.  pool: for the max-pool -- the zeros of
    `signed_zero` have ONE sign per channel (the maximum of +0.0 and -0.0 is either of them: it depends on the order of the scan, which
    nobody promises)."""
    rng = np.random.default_rng(seed * 104729 + int(np.prod(shape)) % 65521 + C)
    x = rng.standard_normal(shape).astype(f32)
    b = rng.standard_normal(C).astype(f32)
    r = rng.standard_normal(shape).astype(f32)
    flat = x.reshape(-1, C)
    if profile == "unit":
        pass
    elif profile == "large":
        x *= f32(1e30)
        b *= f32(1e30)
        r *= f32(1e30)
        with np.errstate(all="ignore"):
            flat[::3] *= f32(3e8)                  # sums that reach +-inf
        x[...] = flat.reshape(shape)
    elif profile == "cancel":
        flat[...] = -b[None]                       # x = -bias exactly ...
        odd = flat[1::2]
        odd[...] = np.nextafter(odd, f32(np.inf) * np.sign(rng.standard_normal(odd.shape)).astype(f32))   # ... and to one ulp
        x = flat.reshape(shape).copy()
        r *= f32(1e-7)
    elif profile == "signed_zero":
        x = np.where(rng.random(shape) < 0.5, f32(-0.0), f32(0.0)).astype(f32)
        b = np.where(np.arange(C) % 2 == 0, f32(-0.0), f32(0.0)).astype(f32)
        r = np.where(rng.random(shape) < 0.5, f32(-0.0), f32(0.0)).astype(f32)
        xf = x.reshape(-1, C)
        xf[:, : max(C // 2, 1)] = f32(-0.0)        # whole channels of -0.0 + -0.0
        if pool:
            xf[:, max(C // 2, 1):] = np.where(np.arange(C - max(C // 2, 1)) % 3 == 0, f32(-0.0), f32(0.0))[None]
        x = xf.reshape(shape).copy()
    elif profile == "non_finite":
        k = rng.random(shape)
        x[k < 0.02] = np.nan
        x[(k >= 0.02) & (k < 0.04)] = np.inf
        x[(k >= 0.04) & (k < 0.06)] = -np.inf
        r[(k >= 0.5) & (k < 0.51)] = np.inf        # inf + -inf as well
        r[(k >= 0.03) & (k < 0.05)] = -np.inf
        if C >= 8:
            b[C - 1] = np.nan
            b[1] = np.inf
    else:
        raise ValueError(profile)
    return np.ascontiguousarray(x), b, r


# ---- bit comparison --------------------------------------------------------------------------------------------------------------
def bits_differ(a, b):
    """Number of elements of two fp32 arrays that differ: NaN against NaN is equal (payloads are not compared), every other pair is
    compared bit for bit (so +0.0 != -0.0)."""
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    return int(np.count_nonzero((na != nb) | (~na & ~nb & (a.view(np.int32) != b.view(np.int32)))))


def values_differ(a, b):
    """As bits_differ, but +0.0 equals -0.0: for a comparison with an implementation whose zeros' signs are its own."""
    a, b = np.ascontiguousarray(a, dtype=f32), np.ascontiguousarray(b, dtype=f32)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    return int(np.count_nonzero((na != nb) | (~na & ~nb & (a != b))))


def against_device_chain(got, chain, profile):
    """(elements that differ from the torch chain on the device, zeros among them whose only difference is the sign).  Outside the
    `signed_zero` profile every bit counts; in it the values must agree and the signs of zeros are reported, not asserted: the kernels are
    pinned to `v < 0 ? 0 : v` (the float64-rounded-once reference, torch's CPU relu), which keeps -0.0, while the element-wise ATen
    kernels on the device return +0.0 for relu(-0.0)."""
    bits = bits_differ(got, chain)
    if profile != "signed_zero":
        return bits, 0
    vals = values_differ(got, chain)
    return vals, bits - vals


def _relu(v):
    """`v < 0 ? 0 : v`: keeps -0.0 and NaN."""
    return np.where(v < 0, f32(0), v).astype(f32)


def _round(v64):
    with np.errstate(all="ignore"):
        return np.asarray(v64, dtype=np.float64).astype(f32)


# ---- the additive kernels: float64 rounded once, and fp32 models with mutants -----------------------------------------------------------
def bias_act_reference(x, b, r=None, relu=True):
    """x [..., C]: round(round(x + b) + r), then ReLU; formed in float64, rounded after each addition."""
    with np.errstate(all="ignore"):
        v = _round(x.astype(np.float64) + b.astype(np.float64))
        if r is not None:
            v = _round(v.astype(np.float64) + r.astype(np.float64))
    return _relu(v) if relu else v


def bias_act_f32(x, b, r=None, relu=True, mutant=None):
    C = b.size
    if mutant == "bias_quad_off_by_one":
        b = b[(np.arange(C) + 4) % C]
    with np.errstate(all="ignore"):
        v = x + b
        if r is not None:
            v = v + r
    return _relu(v) if relu else v


def _pool3x3s2p1(v):
    """max over 3 x 3 / stride 2 / padding 1 windows of v [N, H, W, C]; a NaN in the window is the maximum (torch.max_pool2d)."""
    N, H, W, C = v.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), -np.inf, v.dtype)
    p[:, 1:H + 1, 1:W + 1] = v
    taps = [p[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2] for dy in range(3) for dx in range(3)]
    return np.max(np.stack(taps), axis=0)          # np.max propagates NaN


def maxpool_reference(x, b):
    """x [N, H, W, C] -> maxpool3x3/s2/p1(relu(round(x + b)))."""
    with np.errstate(all="ignore"):
        return _pool3x3s2p1(_relu(_round(x.astype(np.float64) + b.astype(np.float64))))


def maxpool_f32(x, b, mutant=None):
    with np.errstate(all="ignore"):
        if mutant == "relu_before_bias":
            v = _relu(x) + b
        else:
            v = _relu(x + b)
        if mutant == "nan_dropped":            # `v > m ? v : m` from the window's centre: only the centre's NaN survives
            N, H, W, C = v.shape
            Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            centre = v[:, ::2, ::2]
            rest = _pool3x3s2p1(np.where(np.isnan(v), f32(-np.inf), v))
            return np.where(np.isnan(centre), centre, rest).astype(f32)
        if mutant == "window_no_pad_shift":    # rows 2 oy .. 2 oy + 2
            N, H, W, C = v.shape
            Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
            p = np.full((N, 2 * Ho + 2, 2 * Wo + 1, C), -np.inf, f32)
            p[:, :H, 1:W + 1] = v
            taps = [p[:, dy:dy + 2 * Ho:2, dx:dx + 2 * Wo:2] for dy in range(3) for dx in range(3)]
            return np.max(np.stack(taps), axis=0)
        return _pool3x3s2p1(v)


def upsample_add_reference(low, fpn, q_per_image, exact_index=False, in_f32=False):
    """low [N, h, w, C], fpn [N / q, H, W, C] -> round(low[n, ys, xs] + fpn[n / q]) with torch's legacy nearest index."""
    N, h, w, C = low.shape
    _, H, W, _ = fpn.shape
    ys, xs = nearest_index(H, h, exact_index), nearest_index(W, w, exact_index)
    up = low[:, ys][:, :, xs]
    fp = fpn[np.arange(N) // q_per_image]
    with np.errstate(all="ignore"):
        if in_f32:
            return up + fp
        return _round(up.astype(np.float64) + fp.astype(np.float64))


def upsample_add_f32(low, fpn, q_per_image, mutant=None):
    return upsample_add_reference(low, fpn, q_per_image, exact_index=mutant == "exact_nearest", in_f32=True)


# ---- post-processing: fp32 model, float64 rule ---------------------------------------------------------------------------------------
def _sigmoid_f32(v):
    with np.errstate(all="ignore"):
        return (f32(1) / (f32(1) + np.exp(-v.astype(f32)))).astype(f32)


def postprocess_boxes_f32(boxes, img_h, img_w, clip, mutant=None):
    """The documented box arithmetic, one fp32 rounding per operation."""
    ih, iw = f32(img_h), f32(img_w)
    if mutant == "swap_xy":
        ih, iw = iw, ih
    cx, cy, bw, bh = (boxes[:, k].astype(f32) for k in range(4))
    with np.errstate(all="ignore"):
        hw, hh = f32(0.5) * bw, f32(0.5) * bh
        out = [(cx - hw) * iw, (cy - hh) * ih, (cx + hw) * iw, (cy + hh) * ih]
        if clip:
            sx, sy = (iw - 1, ih - 1) if mutant == "clip_side_minus_1" else (iw, ih)
            # fminf(fmaxf(v, 0), side): a NaN coordinate becomes 0 (fmaxf returns the other operand)
            out = [np.fmin(np.fmax(o, f32(0)), s) for o, s in zip(out, (sx, sy, sx, sy))]
    return np.stack(out, 1).astype(f32)


def postprocess_f32(logits, boxes, img_h, img_w, clip, mutant=None):
    """[Q, 6] of the documented operation in fp32: score = max_c sigmoid, label = the first class that attains it; a NaN score counts
    as the maximum and the first NaN class keeps it (torch.max)."""
    s = _sigmoid_f32(logits)
    if mutant == "fp16_logit":
        s = _sigmoid_f32(logits.astype(np.float16).astype(f32))
    best, label = s[:, 0].copy(), np.zeros(len(s), np.int64)
    for c in range(1, s.shape[1]):
        if mutant == "label_last_max":
            upd = s[:, c] >= best
        elif mutant == "nan_skipped":
            upd = s[:, c] > best
        else:
            upd = (s[:, c] > best) | (np.isnan(s[:, c]) & ~np.isnan(best))
        best, label = np.where(upd, s[:, c], best), np.where(upd, c, label)
    return np.concatenate([postprocess_boxes_f32(boxes, img_h, img_w, clip, mutant), best[:, None], label[:, None].astype(f32)], 1).astype(f32)


class PostVerdict:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __str__(self):
        return ("score/tol %.3f (fp32 torch %.3f) at q %d | labels off the float64 argmax %d (all ambiguous: %s) | ambiguous %.2e | "
                "violations %d | boxes: bits off %d, worst / 2 ulp %.3f" % (self.score_ratio, self.fp32_ratio, self.where, self.differ,
                                                                           self.differ_ambiguous, self.ambiguous, self.violations,
                                                                           self.box_bits, self.box_ratio))

    @property
    def ok(self):
        return (self.violations == 0 and self.differ_ambiguous and self.score_ratio <= 1.0 and self.box_bits == 0 and self.box_ratio <= 1.0
                and self.score_norm <= max(FP32_FACTOR * self.fp32_norm, FP32_CLASS_MIN) and self.nan_mismatch == 0)


def post_reference(logits):
    """float64 side of the label rule: (p64, tol, lo, hi, argmax64, acceptable [Q, C], ambiguous [Q], nan [Q])."""
    l64 = logits.astype(np.float64)
    with np.errstate(all="ignore"):
        p = 1.0 / (1.0 + np.exp(-l64))
    tol = np.where(np.isinf(l64), 0.0, C_TOL * (1 + np.abs(l64)))
    nan = np.isnan(p).any(1)
    pz, tz = np.where(np.isnan(p), -1.0, p), np.where(np.isnan(p), 0.0, tol)
    lo = (pz - tz).max(1)
    acc = pz + tz >= lo[:, None]
    return p, tol, np.argmax(pz, 1), acc, (acc.sum(1) > 1) & ~nan, nan


def post_ambiguous_share(logits):
    return float(post_reference(logits)[4].mean())


def post_check(out, logits, boxes, img_h, img_w, clip, fp32_scores=None):
    """The rules of the module docstring for one [Q, 6] result -> PostVerdict (`.ok`).  fp32_scores: torch's fp32 sigmoid().max(-1)
    scores on the same logits (the fp32 formulation's own error); default: the numpy model's."""
    out = np.asarray(out, dtype=f32)
    Q, C = logits.shape
    p, tol, arg64, acc, amb, nan = post_reference(logits)
    label = out[:, 5].astype(np.int64)
    in_range = (out[:, 5] == label) & (label >= 0) & (label < C)
    lab = np.where(in_range, label, 0)
    rows = np.arange(Q)
    # NaN contract: score NaN, label = the first NaN class
    first_nan = np.argmax(np.isnan(p), 1)
    nan_mismatch = int(np.count_nonzero(np.isnan(out[:, 4]) != nan) + np.count_nonzero(nan & (label != first_nan)))
    fin = ~nan
    viol = int(np.count_nonzero(~in_range) + np.count_nonzero(fin & ~acc[rows, lab]))
    differ = fin & (lab != arg64)
    with np.errstate(all="ignore"):
        err = np.where(fin, np.abs(out[:, 4].astype(np.float64) - p[rows, lab]), 0.0)
        if fp32_scores is None:
            fp32_scores = postprocess_f32(logits, boxes, img_h, img_w, clip)[:, 4]
        p_best = np.where(fin, np.where(np.isnan(p), -1.0, p).max(1), 0.0)
        err32 = np.where(fin, np.abs(np.asarray(fp32_scores, dtype=np.float64) - p_best), 0.0)
    t = np.where(fin, tol[rows, lab], 1.0)
    t = np.where(t > 0, t, U)       # (+-inf logits: tol 0 -- the score must be exact; err / U keeps the ratio finite)
    norm = 1 + np.where(np.isfinite(logits[rows, lab]), np.abs(logits[rows, lab].astype(np.float64)), 0.0)
    k = int(np.argmax(err / t))
    # boxes
    want = postprocess_boxes_f32(boxes, img_h, img_w, clip)
    box_bits = bits_differ(out[:, :4], want)
    b64 = boxes.astype(np.float64)
    with np.errstate(all="ignore"):
        r64 = np.stack([(b64[:, 0] - 0.5 * b64[:, 2]) * img_w, (b64[:, 1] - 0.5 * b64[:, 3]) * img_h,
                        (b64[:, 0] + 0.5 * b64[:, 2]) * img_w, (b64[:, 1] + 0.5 * b64[:, 3]) * img_h], 1)
        if clip:
            r64 = np.clip(r64, 0.0, np.array([img_w, img_h, img_w, img_h], dtype=np.float64))
        side = np.array([img_w, img_h, img_w, img_h], dtype=np.float64)
        okb = np.isfinite(r64) & np.isfinite(out[:, :4])
        box_ratio = float(np.max(np.where(okb, np.abs(out[:, :4].astype(np.float64) - r64) / (BOX_ULPS * np.maximum(np.abs(r64), side)), 0.0)))
    t32 = np.where(fin, tol[rows, arg64], 1.0)
    t32 = np.where(t32 > 0, t32, U)
    return PostVerdict(score_ratio=float((err / t)[k]), where=k, fp32_ratio=float(np.max(err32 / t32)), score_norm=float(np.max(err / norm)),
                       fp32_norm=float(np.max(err32 / norm)), differ=int(differ.sum()), differ_ambiguous=bool(np.all(amb[differ])),
                       ambiguous=float(amb.mean()), violations=viol, box_bits=box_bits, box_ratio=box_ratio, nan_mismatch=nan_mismatch,
                       ambiguous_mask=amb)


# ---- the label map: fp32 model with mutants ----------------------------------------------------------------------------------------------
LABEL_MUTANTS = ["exact_nearest", "align_corners", "skip_nearest", "pad_is_img", "no_clamp", "ge_threshold", "ties_last", "order_ignored",
                 "minus1_row0", "fp16_logit", "saturated_by_logit", "nan_skipped"]
POST_MUTANTS = ["swap_xy", "clip_side_minus_1", "label_last_max", "fp16_logit", "nan_skipped"]
POOL_MUTANTS = ["window_no_pad_shift", "relu_before_bias", "nan_dropped"]


def label_map_f32(logits, order, pad, img, out, thr=0.5, mutant=None):
    """The documented operation in numpy fp32, one rounding per operation -> int16 [out_h, out_w]."""
    logits = np.ascontiguousarray(logits, dtype=f32)
    n, h, w = logits.shape
    g = Geometry(h, w, pad, img, out, mutant)
    flat = logits.reshape(-1)
    o00 = g.y0[:, None] * w + g.x0[None, :]
    o01, o10 = o00 + g.xp[None, :], o00 + g.yp[:, None] * w
    o11 = o10 + g.xp[None, :]
    ly0, ly1, lx0, lx1 = g.ly0[:, None], g.ly1[:, None], g.lx0[None, :], g.lx1[None, :]
    best, bestv = np.full(g.out, -1, f32), np.full(g.out, -np.inf, f32)
    owner = np.full(g.out, -1, np.int64)
    with np.errstate(all="ignore"):
        for t, row in enumerate(order):
            if mutant == "order_ignored":
                row = t % n
            if row < 0:
                if mutant != "minus1_row0":
                    continue
                row = 0
            a, b, c, d = (flat[(row * h * w + o) % flat.size] for o in (o00, o01, o10, o11))   # (% size: the no_clamp mutant's reads)
            v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)
            if mutant == "fp16_logit":
                v = v.astype(np.float16).astype(f32)
            prob = f32(1) / (f32(1) + np.exp(-v))
            if mutant == "ties_last":
                upd = (prob >= best) | np.isnan(prob)
            elif mutant == "saturated_by_logit":
                upd = (prob > best) | ((prob == best) & (v > bestv)) | np.isnan(prob)
            elif mutant == "nan_skipped":
                upd = prob > best
            else:
                upd = (prob > best) | np.isnan(prob)
            best, bestv, owner = np.where(upd, prob, best), np.where(upd, v, bestv), np.where(upd, t, owner)
        keep = (best >= f32(thr)) if mutant == "ge_threshold" else (best > f32(thr))
    return np.where((owner >= 0) & keep, owner, -1).astype(np.int16)


# ---- the label map: the float64 rule (torch: runs where the logits live) -----------------------------------------------------------------
class LabelVerdict:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __str__(self):
        return ("violations %d (first at %s) | ambiguous %.2e | pixels off the float64 argmax %d (all ambiguous: %s) | NaN pixels %d | "
                "owned %.2f" % (self.violations, self.where, self.ambiguous, self.differ, self.differ_ambiguous, self.nan_pixels, self.owned))

    @property
    def ok(self):
        return self.violations == 0 and self.differ_ambiguous


def _canonical_rows(L, order):
    """row -> the first row of L (among those `order` uses) that holds the same bits."""
    used = sorted({int(r) for r in order if r >= 0})
    if not used:
        return {}
    idx = torch.tensor(used, device=L.device)
    finger = torch.stack([L[idx].nan_to_num(nan=7.0, posinf=11.0, neginf=-13.0).sum((1, 2)), L[idx, 0, 0].nan_to_num(nan=7.0, posinf=11.0, neginf=-13.0)], 1).cpu().numpy()
    canon, groups = {}, {}
    for r, fp in zip(used, map(tuple, finger)):
        for c in groups.get(fp, []):
            if torch.equal(L[r].nan_to_num(nan=7.0), L[c].nan_to_num(nan=7.0)):
                canon[r] = c
                break
        else:
            canon[r] = r
            groups.setdefault(fp, []).append(r)
    return canon


def _track_probs(L, order, g, dev):
    """Yields (t, p64, tol) per track with a mask: [out_h, out_w] float64 on `dev`."""
    ti = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    y0, y1, x0, x1 = ti(g.y0), ti(g.y0 + g.yp), ti(g.x0), ti(g.x0 + g.xp)
    ly0, ly1 = ti(g.ly0.astype(np.float64))[:, None], ti(g.ly1.astype(np.float64))[:, None]
    lx0, lx1 = ti(g.lx0.astype(np.float64))[None, :], ti(g.lx1.astype(np.float64))[None, :]
    seen = set()
    canon = _canonical_rows(L, order)
    for t, row in enumerate(order):
        if row < 0 or canon[row] in seen:   # a track whose logits are bitwise those of an earlier track can never win (`>`): left out,
            continue                        # so it is never acceptable
        seen.add(canon[row])
        P = L[row]
        r0, r1 = P.index_select(0, y0), P.index_select(0, y1)
        a, b, c, d = r0.index_select(1, x0), r0.index_select(1, x1), r1.index_select(1, x0), r1.index_select(1, x1)
        v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)
        Sv = ly0 * (lx0 * a.abs() + lx1 * b.abs()) + ly1 * (lx0 * c.abs() + lx1 * d.abs())
        p = torch.sigmoid(v)
        tol = torch.where(torch.isinf(v), torch.zeros_like(v), C_TOL * (1 + Sv))
        tol = torch.where(torch.isnan(tol), torch.zeros_like(tol), tol)
        yield t, p, tol


def label_check(got, logits, order, pad, img, out, thr=0.5, rows=None):
    """The decision rule for one label map.  logits: torch fp32 [n, h, w] (any device; the float64 work runs there), got: int16 [out_h,
    out_w] (tensor or array) or None -- then the float64 decision itself is judged (the ambiguous share of the reference alone).
    rows: judge these output rows only (a sample of a large map, for the CPU)."""
    dev = logits.device
    n, h, w = logits.shape
    g = Geometry(h, w, pad, img, out)
    L = logits.double()
    if rows is not None:
        rows = np.asarray(rows)
        g.y0, g.yp, g.ly0, g.ly1 = g.y0[rows], g.yp[rows], g.ly0[rows], g.ly1[rows]
        if got is not None:
            got = torch.as_tensor(got)[torch.from_numpy(rows)]
    shape = (len(g.y0), int(out[1]))
    lo = torch.full(shape, -math.inf, dtype=torch.float64, device=dev)
    hi, pmax = lo.clone(), lo.clone()
    arg = torch.full(shape, -1, dtype=torch.int64, device=dev)
    nan = torch.zeros(shape, dtype=torch.bool, device=dev)
    for t, p, tol in _track_probs(L, order, g, dev):
        isn = torch.isnan(p)
        nan |= isn
        p = torch.where(isn, torch.full_like(p, -1.0), p)
        lo, hi = torch.maximum(lo, p - tol), torch.maximum(hi, p + tol)
        upd = p > pmax
        pmax, arg = torch.where(upd, p, pmax), torch.where(upd, torch.full_like(arg, t), arg)
    dec64 = torch.where((pmax > thr) & ~nan, arg, torch.full_like(arg, -1))
    gt = dec64 if got is None else torch.as_tensor(got).to(dev).long().reshape(shape)
    n_acc = torch.zeros(shape, dtype=torch.int32, device=dev)
    got_ok = torch.zeros(shape, dtype=torch.bool, device=dev)
    for t, p, tol in _track_probs(L, order, g, dev):
        a = torch.where(torch.isnan(p), torch.full_like(p, -1.0), p) + tol >= lo
        n_acc += a.int()
        got_ok |= a & (gt == t)
    clear_above, clear_below = lo > thr, hi < thr
    bad = torch.where(nan, gt != -1, ((gt == -1) & clear_above) | ((gt != -1) & (clear_below | ~got_ok)))
    amb = ~nan & ~clear_below & ((n_acc > 1) | ~clear_above)
    differ = gt != dec64
    where = None
    if bool(bad.any()):
        k = int(torch.nonzero(bad.reshape(-1))[0])
        where = (k // shape[1], k % shape[1], int(gt.reshape(-1)[k]), int(dec64.reshape(-1)[k]))
    return LabelVerdict(violations=int(bad.sum()), where=where, ambiguous=float(amb.double().mean()), differ=int(differ.sum()),
                        differ_ambiguous=bool((amb | ~differ).all()), nan_pixels=int(nan.sum()), owned=float((dec64 >= 0).double().mean()),
                        decision=dec64)


def torch_label_chain(logits, order, pad, img, out, thr=0.5):
    """The chain the kernel replaces, in torch fp32 on the logits' device: bilinear to the padded size, sigmoid, crop, nearest to the
    output size, stack (a track without a mask: -1 everywhere), max over the tracks, threshold."""
    import torch.nn.functional as F
    cur = F.interpolate(logits[None], size=tuple(pad), mode="bilinear", align_corners=False)[0].sigmoid()
    seg = F.interpolate(cur[:, :img[0], :img[1]].unsqueeze(1), size=tuple(out), mode="nearest").squeeze(1)
    probs = torch.stack([seg[r] if r >= 0 else torch.full(tuple(out), -1.0, device=logits.device) for r in order])
    best, owner = probs.max(dim=0)
    return torch.where(best > thr, owner, torch.full_like(owner, -1)).to(torch.int16)


def order_of(n, kind="identity", seed=0):
    if kind == "identity":
        return list(range(n))
    rng = np.random.default_rng(seed + n)
    order = rng.permutation(n).tolist()
    if kind == "holes" and n > 1:
        order[0] = -1
    return order


# ---- exact profiles: saturation, ties, the threshold itself, NaN ------------------------------------------------------------------------
def exact_label_cases():
    """(name, logits, order, pad, img, out, thr, expected map or a predicate) -- inputs on which fp32 leaves no margin to argue about."""
    lw, pad, img, out = (13, 21), (52, 84), (50, 84), (67, 107)
    n = 6
    cases = []
    full = lambda v: np.full(out, v, np.int16)
    cases.append(("zero: 0.5 is not > 0.5", label_logits("zero", n, *lw), order_of(n), 0.5, full(-1)))
    cases.append(("zero at thr 0.3: first track", label_logits("zero", n, *lw), [-1, 2, 0, 1], 0.3, full(1)))
    cases.append(("subnormal: all exactly 0.5", label_logits("subnormal", n, *lw), order_of(n), 0.5, full(-1)))
    cases.append(("subnormal at thr 0.3: first track", label_logits("subnormal", n, *lw), [-1, -1, 4, 1], 0.3, full(2)))
    cases.append(("saturated: all exactly 1.0, first track", label_logits("saturated", n, *lw), [-1, 5, 0, 3], 0.5, full(1)))
    cases.append(("threshold 0.0: every probability is above it", label_logits("neg", n, *lw), order_of(n), 0.0, None))
    cases.append(("order all -1", label_logits("unit", n, *lw), [-1, -1, -1], 0.5, full(-1)))
    return [(name, x, order, pad, img, out, thr, want) for name, x, order, thr, want in cases]


def check_exact_label_cases(run):
    """run(logits, order, pad, img, out, thr) -> int16 map.  Also: equal rows (the first track wins everywhere), a NaN / inf contract."""
    for name, x, order, pad, img, out, thr, want in exact_label_cases():
        got = np.asarray(run(x, order, pad, img, out, thr))
        if want is not None:
            assert np.array_equal(got, want), name
        else:
            v = label_check(got, torch.from_numpy(x), order, pad, img, out, thr)
            assert v.ok and not (got == -1).any(), name
    # two tracks on one row, and two bitwise equal rows: the first in order wins
    lw, pad, img, out = (13, 21), (52, 84), (50, 84), (67, 107)
    x = label_logits("unit", 6, *lw)
    x[4] = x[1]
    order = [3, 1, -1, 3, 4, 0, 1]
    got = np.asarray(run(x, order, pad, img, out, 0.5))
    v = label_check(got, torch.from_numpy(x), order, pad, img, out, 0.5)
    assert v.ok, str(v)
    assert (got == 0).any() and (got == 1).any() and not np.isin(got, [3, 4, 6]).any(), "equal rows: not the first track"
    assert np.array_equal(got, v.decision.numpy().astype(np.int16)) or v.differ_ambiguous


def nan_label_case(kind):
    """Logits with one non-finite value per track row in different places, incl. a corner that carries bilinear weight exactly 0."""
    lw, pad, img, out = (8, 9), (32, 36), (32, 36), (32, 36)
    x = label_logits("unit", 4, *lw, seed=3)
    val = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[kind]
    x[0, 3, 4] = val            # first track
    x[2, 6, 1] = val            # a later track
    x[1, 0, 0] = val            # the clamped corner: weights exactly (1, 0) along both axes for the first output pixels
    x[3, 7, 8] = val            # the last row / column: the second tap is the first (yp = xp = 0)
    return x, [0, 1, 2, 3], pad, img, out


def check_nan_label_contract(run):
    for kind in ("nan", "+inf", "-inf"):
        x, order, pad, img, out = nan_label_case(kind)
        got = np.asarray(run(x, order, pad, img, out, 0.5))
        want = torch_label_chain(torch.from_numpy(x), order, pad, img, out, 0.5).numpy()
        v = label_check(got, torch.from_numpy(x), order, pad, img, out, 0.5)
        print("DECISION label map with %s: %s; differs from the torch chain on %d pixels" % (kind, v, int((got != want).sum())))
        assert v.ok, (kind, str(v))
        if kind != "-inf":
            assert v.nan_pixels > 0      # (0 * inf at the zero-weight taps as well)
        vt = label_check(want, torch.from_numpy(x), order, pad, img, out, 0.5)
        assert vt.ok, (kind, str(vt))
        amb = int(round(v.ambiguous * got.size))
        assert int((got != want).sum()) <= amb
