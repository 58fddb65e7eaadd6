"""The float64 yardstick of the backward of out = LayerNorm(x + res) gamma + beta (trackformer_amd/csrc/layernorm_bwd.h; include/tf_fused.h:
THE BACKWARD OF THE RESIDUAL LAYERNORM) and the gradient profiles its tests draw dy from.  x / res / gamma / beta come from
tests/util_norm_attn_numerics.norm_operands; the constants and the reporting (Excess) are the project's.

From the fp32 operands, in float64: z = x + res, mean, the biased variance, rstd = 1 / sqrt(var + eps), xh = (z - mean) rstd, g = gamma dy,

    ref_dz = rstd (g - mean_c g - xh mean_c(g xh))        ref_dgamma = sum_r dy xh        ref_dbeta = sum_r dy

    dz,     per element   (|dz - ref| - 4 . 2^-149) / S_z   <=  2^-20         S_z = rstd (|g| + mean_c |g| + X mean_c(|g| X))
    dgamma, per column    |dgamma - ref| / sum_r |dy| X     <=  bound_for(rows)
    dbeta,  per column    |dbeta - ref| / sum_r |dy|        <=  bound_for(rows)

X = rstd (|z - mean| + |mean|) is the LayerNorm yardstick's scale of an error in xh (it covers the fp32 rounding of `mean`);
bound_for(rows) is 2^-20, growing as sqrt(rows / 1152) beyond 1152 rows (fp32 accumulation over the rows).  Second criterion, as
everywhere in this project: the kernel's worst normalised excess is at most 4 x that of torch's own fp32 formulation -- autograd through
F.layer_norm(x + res) -- on the same operands, or FP32_CLASS_MIN where that is as good as exact.  No element is exempt.

Everything here is torch, float64, and runs on the CPU or the device."""
import torch
import torch.nn.functional as F

from tests import util_norm_attn_numerics as NA
from tests import util_split_numerics as U

DY_PROFILES = ["unit", "spread", "row_spread", "tiny", "big"]
EPS = 1e-5
OUTPUTS = ("dz", "dgamma", "dbeta")


def dy_operand(profile, rows, C, seed, device="cpu"):
    """Seeded dy [rows, C] for `profile`."""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(rows, C, generator=g)
    if profile == "spread":          # per element 2^+-12, one in ten exactly zero
        dy *= torch.exp2(torch.randint(-12, 13, (rows, C), generator=g).float())
        dy[torch.rand(rows, C, generator=g) < 0.1] = 0.0
    elif profile == "row_spread":    # per row 2^+-12: the column sums mix rows of very different weight
        dy *= torch.exp2(torch.randint(-12, 13, (rows, 1), generator=g).float())
    elif profile == "tiny":
        dy *= 1e-6
    elif profile == "big":
        dy *= 1e3
    elif profile != "unit":
        raise ValueError(profile)
    return dy.to(device)


def operands(profile, dy_profile, rows, C, seed, device="cpu", with_res=None):
    """(x [rows, C], res or None, gamma, beta, dy).  with_res True: a res for the profiles that bring none (unit-scale noise); False:
    none, whatever the profile brings; None: as the profile has it (`cancel` only)."""
    x, res, gamma, beta = NA.norm_operands(profile, 1, rows, C, seed, device)
    x = x.reshape(rows, C)
    res = None if res is None else res.reshape(rows, C)
    if with_res is True and res is None:
        res = torch.randn(rows, C, generator=torch.Generator().manual_seed(seed + 7919)).to(device)
    elif with_res is False:
        res = None
    return x, res, gamma, beta, dy_operand(dy_profile, rows, C, seed + 104729, device)


def reference(x, res, gamma, dy, eps=EPS):
    """{"dz" | "dgamma" | "dbeta": NA.Ref(ref, scale, floor)} in float64 on the operands' device."""
    z = x.double() if res is None else x.double() + res.double()
    mean = z.mean(-1, keepdim=True)
    var = z.var(-1, unbiased=False, keepdim=True)
    rstd = 1.0 / (var + eps).sqrt()
    xh = (z - mean) * rstd
    d = dy.double()
    g = gamma.double() * d
    ref_dz = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    X = rstd * ((z - mean).abs() + mean.abs())
    S_z = rstd * (g.abs() + g.abs().mean(-1, keepdim=True) + X * (g.abs() * X).mean(-1, keepdim=True))
    zero = torch.zeros_like(gamma, dtype=torch.float64)
    return {"dz": NA.Ref(ref_dz, S_z, torch.full_like(ref_dz, 4 * NA.SUB)),
            "dgamma": NA.Ref((d * xh).sum(0), (d.abs() * X).sum(0), zero),
            "dbeta": NA.Ref(d.sum(0), d.abs().sum(0), zero)}


def fp32_formulation(x, res, gamma, beta, dy, eps=EPS):
    """torch's own fp32 formulation on the operands' device: autograd through F.layer_norm(x + res) -> (dz, dgamma, dbeta)."""
    with torch.enable_grad():
        xl = x.detach().clone().requires_grad_(True)
        gl, bl = gamma.detach().clone().requires_grad_(True), beta.detach().clone().requires_grad_(True)
        z = xl if res is None else xl + res
        y = F.layer_norm(z, (x.shape[-1],), gl, bl, eps)
        dz, dg, db = torch.autograd.grad(y, (xl, gl, bl), dy)
    return {"dz": dz, "dgamma": dg, "dbeta": db}


def bound(name, rows):
    return U.BOUND if name == "dz" else U.bound_for(rows)


def excess_of(name, got, ref, fp32=None):
    """The worst element (Excess) of one output against its Ref; fp32: torch's fp32 result, reported on the Excess."""
    _, worst = NA.excess(got, ref[name], None if fp32 is None else fp32[name])
    return worst


def check(got, ref, fp32, rows, what=""):
    """Assert both criteria for every output in `got` ({name: tensor}); prints each worst excess next to the fp32 formulation's own
    (pytest -s) before it asserts.  Returns {name: Excess}."""
    out = {}
    for name in OUTPUTS:
        if got.get(name) is None:
            continue
        worst = excess_of(name, got[name], ref, fp32)
        out[name] = worst
        print("%-52s %-6s %.3e (torch fp32: %.3e, bound %.3e)" % (what, name, worst.value, worst.fp32_err, bound(name, rows)))
    for name, worst in out.items():
        assert worst.value <= bound(name, rows), (what, name, worst)
        assert worst.value <= max(NA.FP32_FACTOR * worst.fp32_err, NA.FP32_CLASS_MIN), (what, name, worst)
    return out


def check_fp32_alone(ref, fp32, rows, what=""):
    """The fp32 formulation itself stays inside the bounds (the yardstick is one an fp32 implementation can meet)."""
    out = {}
    for name in OUTPUTS:
        worst = excess_of(name, fp32[name], ref)
        out[name] = worst
        print("%-52s %-6s torch fp32 %.3e (bound %.3e)" % (what, name, worst.value, bound(name, rows)))
        assert worst.value <= bound(name, rows), (what, name, worst)
    return out
