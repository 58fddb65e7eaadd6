"""The generator contract of the dropout inside the training kernels (include/tf_fused.h: DROPOUT INSIDE THE TRAINING KERNELS;
trackformer_amd/csrc/dropout_rng.h), restated in numpy, and the float64 yardstick of out = LayerNorm(x + keep scale res) gamma + beta and
its backward (trackformer_amd/csrc/dropout_train.h).

THE CONTRACT.  Philox4x32-10, key (seed low, seed high), counter (g low, g high, offset low, offset high) for the group g of four
consecutive elements of the flat tensor; output word j decides element 4 g + j: kept iff word >= T = floor(p 2^32) (p the float, the
product in double); survivors are multiplied by the float 1.0f / (1.0f - p).

THE YARDSTICK is that of tests/util_layernorm_train.py with one more operand.  From the fp32 operands and the mask, in float64, with the
EXACT scale s = 1 / (1 - p) (p the float):  d = keep s res,  z = x + d,  mean, rstd, xh, g = gamma dy as there, and

    ref_out = xh gamma + beta      ref_dx = rstd (g - mean_c g - xh mean_c(g xh))      ref_dres = keep s ref_dx
    ref_dgamma = sum_r dy xh       ref_dbeta = sum_r dy

The kernel's d carries two fp32 roundings that a plain residual does not -- the scale fl(1 / (1 - p)) and the product fl(scale res) --:
a perturbation delta of z with |delta_i| <= 2 . 2^-24 |d_i| before the sum is formed.  To first order it moves xh_i by
rstd (delta_i - mean_c delta) - xh_i rstd mean_c(xh delta), at most rstd 2^-24 . 2 E_i with

    E_i = |d_i| + mean_c |d| + |xh_i| mean_c(|xh| |d|)

so the scale of an error in xh, X = rstd (|z - mean| + |mean|) there, becomes  X = rstd (|z - mean| + |mean| + 2 E)  -- every rounding
of an operand of z is charged at the operand's magnitude, the two of d at theirs, counted from the operations and not from what any
implementation gives.  With it, unchanged in form:

    out,    per element   (|out - ref| - 4 . 2^-149) / (|gamma| X + |beta|)     <= 2^-20
    dx,     per element   (|dx - ref| - 4 . 2^-149) / S_z                        <= 2^-20     S_z = rstd (|g| + mean_c |g| + X mean_c(|g| X))
    dres,   per element   (|dres - ref| - (4 s + 1) 2^-149) / (keep s (S_z + |ref_dx|))  <= 2^-20   (dres = fl(fl(s) dx): the error of dx
                          times s, plus two roundings of |dres| <= s |dx|); where dropped the scale is 0: dres must be exactly 0
    dgamma, per column    |dgamma - ref| / sum_r |dy| X     <= bound_for(rows)
    dbeta,  per column    |dbeta - ref| / sum_r |dy|        <= bound_for(rows)

Second criterion, as everywhere: at most 4 x the worst normalised excess of torch's own fp32 formulation WITH THE SAME MASK -- autograd
through F.layer_norm(x + res keep scale) --, or FP32_CLASS_MIN.  Everything below the restatement is torch and runs on the CPU or the
device."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import util_layernorm_train as Y
from tests import util_norm_attn_numerics as NA
from tests import util_split_numerics as U

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)
EPS = Y.EPS
OUTPUTS = ("out", "dx", "dres", "dgamma", "dbeta")
GRADS = OUTPUTS[1:]


def philox4x32_10(counter, key):
    """counter: four uint32-valued arrays (or scalars) of one shape, key: two -> the four output words, uint32 arrays."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c)).astype(np.uint64) for c in counter)
    k0, k1 = (np.atleast_1d(np.asarray(k)).astype(np.uint64) for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                     # 32 x 32 -> 64 bits: no overflow
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & MASK32, p0 & MASK32, n0, n2
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(p):
    """T = floor(p 2^32): p the float, the product in double."""
    return int(math.floor(float(np.float32(p)) * 4294967296.0))


def scale32(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def scale64(p):
    return 1.0 / (1.0 - float(np.float32(p)))


def words(seed, offset, first, n):
    """The uint32 word of each of the elements first .. first + n - 1 (both multiples of 4) of the stream (seed, offset)."""
    assert first % 4 == 0 and n % 4 == 0
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    g = np.arange(n // 4, dtype=np.uint64) + np.uint64(first // 4)
    w = philox4x32_10((g & MASK32, g >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=1).reshape(-1)


def keep_mask(seed, offset, p, n, first=0):
    """uint8 [n]: 1 where the element is kept."""
    return (words(seed, offset, first, n).astype(np.uint64) >= np.uint64(threshold(p))).astype(np.uint8)


def keep_of(rng, p, shape):
    """The mask of a whole tensor of `shape` from an int64[2] rng tensor (host or device), as a bool tensor on rng's device."""
    seed, offset = (int(v) for v in rng.cpu())
    n = int(np.prod(shape))
    return torch.from_numpy(keep_mask(seed, offset, p, n).astype(bool)).view(*shape).to(rng.device)


# ---- float64 --------------------------------------------------------------------------------------------------------------------------
def reference(x, res, gamma, beta, dy, keep, p, eps=EPS):
    """{"out" | "dx" | "dres" | "dgamma" | "dbeta": NA.Ref(ref, scale, floor)} in float64 on the operands' device; keep: bool [rows, C]."""
    s = scale64(p)
    k = keep.double()
    d = k * s * res.double()
    z = x.double() + d
    mean = z.mean(-1, keepdim=True)
    var = z.var(-1, unbiased=False, keepdim=True)
    rstd = 1.0 / (var + eps).sqrt()
    xh = (z - mean) * rstd
    dd = dy.double()
    ga, be = gamma.double(), beta.double()
    g = ga * dd
    ref_dz = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    E = d.abs() + d.abs().mean(-1, keepdim=True) + xh.abs() * (xh.abs() * d.abs()).mean(-1, keepdim=True)
    X = rstd * ((z - mean).abs() + mean.abs() + 2.0 * E)
    S_z = rstd * (g.abs() + g.abs().mean(-1, keepdim=True) + X * (g.abs() * X).mean(-1, keepdim=True))
    zero = torch.zeros_like(ga)
    ref_out = xh * ga + be
    return {"out": NA.Ref(ref_out, ga.abs() * X + be.abs(), torch.full_like(ref_out, 4 * NA.SUB)),
            "dx": NA.Ref(ref_dz, S_z, torch.full_like(ref_dz, 4 * NA.SUB)),
            "dres": NA.Ref(k * s * ref_dz, k * s * (S_z + ref_dz.abs()), k * ((4 * s + 1) * NA.SUB)),
            "dgamma": NA.Ref((dd * xh).sum(0), (dd.abs() * X).sum(0), zero),
            "dbeta": NA.Ref(dd.sum(0), dd.abs().sum(0), zero)}


def fp32_formulation(x, res, gamma, beta, dy, keep, p, eps=EPS):
    """torch's own fp32 formulation with the same mask: autograd through F.layer_norm(x + res keep scale)."""
    with torch.enable_grad():
        xl, rl = x.detach().clone().requires_grad_(True), res.detach().clone().requires_grad_(True)
        gl, bl = gamma.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
        y = F.layer_norm(xl + rl * keep.float() * float(scale32(p)), (x.shape[-1],), gl, bl, eps)
        dx, dr, dg, db = torch.autograd.grad(y, (xl, rl, gl, bl), dy)
    return {"out": y.detach(), "dx": dx, "dres": dr, "dgamma": dg, "dbeta": db}


def bound(name, rows):
    return U.bound_for(rows) if name in ("dgamma", "dbeta") else U.BOUND


def check(got, ref, fp32, rows, keep=None, what=""):
    """Assert both criteria for every output in `got` ({name: tensor or None}); prints each worst excess next to the fp32 formulation's
    own (pytest -s) before it asserts; dres is also checked to be exactly 0 where dropped.  Returns {name: Excess}."""
    out = {}
    for name in OUTPUTS:
        if got.get(name) is None:
            continue
        _, worst = NA.excess(got[name], ref[name], None if fp32 is None else fp32[name])
        out[name] = worst
        print("%-56s %-6s %.3e (torch fp32: %.3e, bound %.3e)" % (what, name, worst.value, worst.fp32_err, bound(name, rows)))
    if keep is not None and got.get("dres") is not None:
        dropped = ~keep.to(got["dres"].device).reshape(got["dres"].shape)
        assert bool((got["dres"][dropped] == 0).all()), (what, "dres is not exactly 0 where dropped")
    for name, worst in out.items():
        assert worst.value <= bound(name, rows), (what, name, worst)
        assert worst.value <= max(NA.FP32_FACTOR * worst.fp32_err, NA.FP32_CLASS_MIN), (what, name, worst)
    return out


def check_fp32_alone(ref, fp32, rows, what=""):
    """The fp32 formulation itself stays inside the bounds (the yardstick is one an fp32 implementation can meet)."""
    for name in OUTPUTS:
        _, worst = NA.excess(fp32[name], ref[name])
        print("%-56s %-6s torch fp32 %.3e (bound %.3e)" % (what, name, worst.value, bound(name, rows)))
        assert worst.value <= bound(name, rows), (what, name, worst)


def operands(profile, dy_profile, rows, C, seed, device="cpu"):
    """(x, res, gamma, beta, dy) of tests/util_layernorm_train.operands, always with a res."""
    return Y.operands(profile, dy_profile, rows, C, seed, device, with_res=True)
