"""The float64 yardsticks of the attention core's training path (include/tf_fused.h: TRAINING THROUGH THE ATTENTION CORE;
trackformer_amd/csrc/mha_bwd.h), for a GIVEN keep mask, and the mask contract restated in numpy.  Extends attention_reference of
tests/util_norm_attn_numerics.py (NA) by dropout on the weights and by the backward.

THE MASK CONTRACT.  The decision for weight (n, h, i, j) is that of flat element r Lk4 + j of the stream, r = (n H + h) Lq + i,
Lk4 = 4 ceil(Lk / 4): tests/util_dropout_train.keep_mask over N H Lq Lk4 elements, viewed [N, H, Lq, Lk4] and sliced to Lk (keep_mask()).

THE REFERENCE, float64, from the fp32 operands, the key mask and the keep mask, with the EXACT s_p = 1 / (1 - p) (p the float):
    P = softmax_j(scale q . k_j) over the keys the mask leaves,   Pd = keep s_p P,   out = Pd V,
    dP = dout V^T,   delta_i = sum_j Pd_ij dP_ij,   dS = P (keep s_p dP - delta),   dq = scale dS K,   dk = scale dS^T Q,   dv = Pd^T dout

THE YARDSTICKS, per element, bound 2^-20.  T_i = |scale| max_j sum_c |q_ic| |k_jc| is the size of a score sum in nats (NA's T): an fp32
score carries an error of about u T, which moves every weight of the row by P u T -- so each weight, exact or rebuilt, is charged
(1 + T_i).  The scale of an output is the sum of the magnitudes of its terms with that factor on every weight:
    out_i    S (1 + T_i),                      S = sum_j Pd_ij |v_j|             floor 2^-149 (Lk + 2)      (NA's)
    dv_j     sum_i Pd_ij |dout_i| (1 + T_i)                                      floor 2^-149 (Lq + 2 + s_p sum_i |dout_i|)
    dq_i     |scale| sum_j G_ij |k_j|                                            floor 2^-149 (Lk + 2 + |scale| sum_j M_ij |k_j|)
    dk_j     |scale| sum_i G_ij |q_i|                                            floor 2^-149 (Lq + 2 + |scale| sum_i M_ij |q_i|)
    with  A_ij = sum_c |dout_ic| |v_jc|  (the terms of dP_ij),  Delta_i = sum_j Pd_ij A_ij  (the terms of delta_i),
          G_ij = P_ij (keep_ij s_p A_ij + Delta_i) (1 + T_i)   (the terms of dS_ij)   and   M_ij = keep_ij s_p A_ij + Delta_i + 1.
THE FLOORS, corrected.  A first version took the forward's floor with the length of the respective sum, 2^-149 (L + 2).  The fp32 torch
formulation itself missed it (qoffset, dk, 9.6e-7 at an element of 2e-42): the derivation was wrong, not the constant.  The forward's
floor charges 2^-149 per TERM; in the backward a weight that lies in fp32's subnormal range carries an ABSOLUTE error of up to 2^-149
and is then MULTIPLIED: by keep s_p dP - delta (at most M_ij - 1) and by |scale| |k_j| or |scale| |q_i| on its way into dq and dk, by
s_p |dout_i| into dv; the rounding of dS itself adds the 1 in M.  The floor of each output is therefore 2^-149 times the sum of those
multipliers over its terms, on top of the 2^-149 per term.  Masked keys carry no term.
Second criterion as in NA: at most 4 x the worst normalised excess of the fp32 torch formulation WITH THE SAME MASK (autograd through
softmax(scale q k^T) keep s_p v), or 2^-23.

EXACT ZEROS.  Rows whose keys are all masked: out and dq are compared with zero bit for bit, and so are dk and dv of the keys of such an
image (Ref.zero, at most half of an output: NA.excess asserts it).  Masked keys of other images have dk = dv = 0 with scale 0: check()
compares them with zero bit for bit as well.

test_attention_train_cpu.py::test_fp32_formulation_passes_the_yardsticks runs the fp32 formulation alone against these bounds on every
profile of NA.ATTN_PROFILES: a yardstick fp32 cannot meet would be a wrong derivation."""
import math

import numpy as np
import torch

from tests import util_dropout_train as DT
from tests import util_norm_attn_numerics as NA

OUTPUTS = ("out", "dq", "dk", "dv")


def keep_mask(seed, offset, p, N, H, Lq, Lk):
    """bool numpy [N, H, Lq, Lk]: the mask contract."""
    lk4 = 4 * ((Lk + 3) // 4)
    return DT.keep_mask(seed, offset, p, N * H * Lq * lk4).reshape(N, H, Lq, lk4)[..., :Lk].astype(bool)


def keep_of(rng, p, N, H, Lq, Lk):
    """keep_mask() from an int64[2] rng tensor, as a bool tensor on its device."""
    seed, offset = (int(v) for v in rng.cpu())
    return torch.from_numpy(keep_mask(seed, offset, p, N, H, Lq, Lk)).to(rng.device)


def grad_operand(N, Lq, H, D, seed, device="cpu"):
    g = torch.Generator().manual_seed(seed + 77)
    return torch.randn(N, Lq, H, D, generator=g).to(device)


def reference(q, k, v, dout, scale, key_mask=None, keep=None, p=None):
    """q / dout [N, Lq, H, D], k / v [N, Lk, H, D] (fp32), key_mask [N, Lk] or None, keep bool [N, H, Lq, Lk] or None (then p is not
    read) -> {"out" | "dq" | "dk" | "dv": NA.Ref} in the operands' layout, float64."""
    qd, kd, vd, dd = (t.double().permute(0, 2, 1, 3) for t in (q, k, v, dout))      # [N, H, L, D]
    N, H, Lq, D = qd.shape
    Lk = kd.shape[2]
    s = (qd @ kd.transpose(-1, -2)) * scale
    t = (qd.abs() @ kd.abs().transpose(-1, -2)) * abs(scale)
    dead_key = torch.zeros(N, Lk, dtype=torch.bool, device=q.device) if key_mask is None else (key_mask != 0)
    dead = dead_key[:, None, None, :]
    s = s.masked_fill(dead, -math.inf)
    t = t.masked_fill(dead, 0.0)
    dead_img = dead_key.all(-1)                                                      # [N]
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = (s - m).exp()
    den = e.sum(-1, keepdim=True)
    P = e / torch.where(den > 0, den, torch.ones_like(den))
    f = torch.ones_like(P) if keep is None else keep.to(q.device).double() * DT.scale64(p)   # keep s_p
    Pd = f * P
    T1 = 1 + t.amax(-1, keepdim=True)                                                # [N, H, Lq, 1]
    dP = dd @ vd.transpose(-1, -2)
    delta = (Pd * dP).sum(-1, keepdim=True)
    dS = P * (f * dP - delta)
    A = dd.abs() @ vd.abs().transpose(-1, -2)
    Delta = (Pd * A).sum(-1, keepdim=True)
    G = P * (f * A + Delta) * T1
    a = abs(scale)

    def lay(x):
        return x.permute(0, 2, 1, 3).contiguous()

    # floors: a weight in fp32's subnormal range carries an ABSOLUTE error of up to 2^-149, which reaches an output multiplied by
    # whatever multiplies the weight there (M below for dS, s_p |dout| for dv), plus 2^-149 for each term of the sum as in NA
    M = f * A + Delta + 1.0                                                          # (+ 1: the rounding of dS itself)
    sp = 1.0 if keep is None else DT.scale64(p)
    live = (~dead).double()
    fl_dq = NA.SUB * (a * ((M * live) @ kd.abs()) + (Lk + 2))
    fl_dk = NA.SUB * (a * ((M * live).transpose(-1, -2) @ qd.abs()) + (Lq + 2))
    fl_dv = NA.SUB * (sp * dd.abs().sum(-2, keepdim=True).expand(N, H, Lk, D) + (Lq + 2))
    zq = dead_img[:, None, None, None].expand(N, Lq, H, D)
    zk = dead_img[:, None, None, None].expand(N, Lk, H, D)
    fq = NA.SUB * (Lk + 2)

    def ref(x, sc, floor, zero):
        x = lay(x)
        return NA.Ref(x, lay(sc), lay(floor) if torch.is_tensor(floor) else torch.full_like(x, floor), zero)

    return {"out": ref(Pd @ vd, (Pd @ vd.abs()) * T1, fq, zq),
            "dq": ref(scale * (dS @ kd), a * (G @ kd.abs()), fl_dq, zq),
            "dk": ref(scale * (dS.transpose(-1, -2) @ qd), a * (G.transpose(-1, -2) @ qd.abs()), fl_dk, zk),
            "dv": ref(Pd.transpose(-1, -2) @ dd, (Pd * T1).transpose(-1, -2) @ dd.abs(), fl_dv, zk)}


def formulation(q, k, v, dout, scale, key_mask=None, keep=None, p=None, dtype=torch.float32):
    """The torch formulation with the same mask in `dtype`: autograd through softmax(scale q k^T) keep s_p v (NaN where every key of an
    image is masked).  -> {"out", "dq", "dk", "dv"} in the operands' layout."""
    with torch.enable_grad():
        ql, kl, vl = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v))
        s = (ql.permute(0, 2, 1, 3) @ kl.permute(0, 2, 3, 1)) * scale
        if key_mask is not None:
            s = s.masked_fill((key_mask != 0)[:, None, None, :], -math.inf)
        w = torch.softmax(s, -1)
        if keep is not None:
            sp = float(DT.scale32(p)) if dtype == torch.float32 else DT.scale64(p)
            w = w * (keep.to(q.device).to(dtype) * sp)
        out = (w @ vl.permute(0, 2, 1, 3)).permute(0, 2, 1, 3)
        dq, dk, dv = torch.autograd.grad(out, (ql, kl, vl), dout.to(dtype))
    return {"out": out.detach().contiguous(), "dq": dq, "dk": dk, "dv": dv}


def worst(got, ref, fp32=None, what=""):
    """{name: Excess} for every output in `got`; prints each figure (pytest -s)."""
    res = {}
    for name in OUTPUTS:
        if got.get(name) is None:
            continue
        _, w = NA.excess(got[name], ref[name], None if fp32 is None else fp32[name])
        res[name] = w
        print("%-64s %-4s %.3e (torch fp32: %.3e, bound %.3e)" % (what, name, w.value, w.fp32_err, NA.BOUND))
    return res


def check(got, ref, fp32, key_mask=None, what=""):
    """Assert both criteria for every output in `got`, and dk / dv exactly zero at masked keys.  Returns {name: Excess}."""
    res = worst(got, ref, fp32, what)
    if key_mask is not None:
        dead = torch.as_tensor(key_mask != 0)
        for name in ("dk", "dv"):
            if got.get(name) is not None:
                g = torch.as_tensor(got[name]).reshape(ref[name].ref.shape).to(dead.device)
                assert bool((g[dead] == 0).all()), (what, name, "not exactly zero at a masked key")
    for name, w in res.items():
        assert w.value <= NA.BOUND, (what, name, w)
        if fp32 is not None:
            assert w.value <= max(NA.FP32_FACTOR * w.fp32_err, NA.FP32_CLASS_MIN), (what, name, w)
    return res


def check_fp32_alone(ref, fp32, what=""):
    for name in OUTPUTS:
        _, w = NA.excess(fp32[name], ref[name])
        print("%-64s %-4s torch fp32 %.3e (bound %.3e)" % (what, name, w.value, NA.BOUND))
        assert w.value <= NA.BOUND, (what, name, w)


def masks(N, Lk, seed, device="cpu", last_image_dead=False):
    """uint8 [N, Lk]: NA.attention_masks; last_image_dead: every key of the last image masked and none of the others (the exact-zero
    outputs stay within half of each tensor)."""
    if not last_image_dead:
        return NA.attention_masks(N, Lk, seed, device)
    m = torch.zeros(N, Lk, dtype=torch.uint8)
    m[-1] = 1
    return m.to(device)
