"""TEST INFRASTRUCTURE of tests/test_msda_fused_train_{cpu,gpu}.py: the cases, the float64 restatement and the bounds of the two
kernels that make the fused MSDeformAttn entry trainable (tf_msda_fused_prologue_f32 / tf_msda_fused_backward_epilogue_f32,
include/tf_msda.h; trackformer_amd/csrc/msda_fused_bwd.h).  The yardstick is the one of tests/util_msda_numerics.py (U):

    (|y - ref| - floor) / S  <=  2^-20 sqrt(max(n, 64) / 64)       and exactly the outputs float64 makes NaN are NaN.

Prologue.  Held to U.fused_locations (float64 from the fp32 qproj and reference points): |loc_k - loc| <= dl and
|attn_k - a| <= da with dl, da exactly what that function returns (dl = 2^-22 |off term| + 2^-23 |loc|: a division or a
product good to 1 ulp and the rounded add; da: the __expf / sum / reciprocal budget of U's docstring + 2^-126).

Epilogue.  Held to float64 of its own formulas on the SAME fp32 inputs (a = attn, ga = grad_attn, gl = grad_loc):
    grad_off    gl / (H_l, W_l) or gl ref[2:] 0.5 / P.  One rounded division, or a reciprocal good to 1 ulp (2^-23) and one
                rounded product (2^-24), or -- 4-d -- one rounded product and an exact scaling by a power of two: relative
                2^-23 + 2^-24 < 2^-22 in every form; a result in the fp32 subnormals is good to their spacing 2^-149 only.
                So |y - ref| <= 2^-22 |ref| + 2^-149, element by element, no S.
    grad_logit  a_i (ga_i - sum_j a_j ga_j): a sum of L P + 1 terms (ga_i and the L P products) times a_i.
                S = a_i (|ga_i| + sum_j a_j |ga_j|), n = L P + 1.  Every product a_j ga_j, the subtraction and the final
                product round once more than the sum's own additions; each can land in the subnormals, where it is good to
                2^-149: floor = 2^-149 (L P + 2) (L P products + the difference + the result, the factor a_i <= 1).
    grad_ref[:2]   sum_{m,p} gl: S = sum |gl|, n = M P, no floor (sums of fp32 numbers are exact in the subnormals).
    grad_ref[2:]   sum_{m,p} gl off 0.5 / P: each term is a rounded product, then the sum: S = sum |gl off| 0.5 / P, n = 2 M P
                (M P products + M P additions), no floor; 0.5 / P is a power of two.

Out-of-range samples.  A sample out of range takes no part in the forward, so float64 gives its grad_loc / grad_attn as 0.  The
operator's backward kernels form them as grad_out times zeroed corners: 0 too, but NaN under a NaN in grad_out.  The epilogue
therefore reads the gradients of a sample as 0 when the operator kernels' own range test (one fma per coordinate, in_range
below) on the prologue's own location says "out"; the float64 restatement on the same fp32 inputs does the same with the
same test, which is exact to reproduce.  On gradients an operator kernel wrote from finite inputs this changes nothing.

Left-out coordinates.  U.backward_reference leaves the grad_loc coordinates within 2 dx of a cell edge out of its comparison
(grad_loc jumps there); the same coordinates are left out of grad_off wherever grad_off is computed from a KERNEL's grad_loc and
compared with float64's (the end-to-end test).  On the same fp32 inputs nothing is left out.  grad_ref is never masked.

End to end the rule is that of tests/test_linear_backward_gpu.py: per tensor e = max |y - ref| / max |ref| against float64, and
e_new <= max(U.FP32_FACTOR * e of today's fp32 module chain on the same inputs, U.FP32_CLASS_MIN)."""
import ctypes

import torch

from tests import util_msda_numerics as U

SEED = 7
PYR = [(25, 42), (13, 21), (7, 11), (4, 6)]
RAGGED16 = [(1, 1), (1, 7), (5, 1), (3, 4), (1, 1), (2, 9), (6, 1), (1, 3), (4, 4), (1, 1), (3, 1), (1, 2), (2, 2), (1, 5),
            (7, 1), (1, 1)]   # tests/test_msda_numerics_gpu.py
S_PYR = sum(h * w for h, w in PYR)

CASES = {   # id -> make_fused_case arguments: the smallest shapes at which the kernels can still go wrong
    "dec_r2": dict(N=2, M=8, D=32, Lq=77, P=4, shapes=PYR, ref_dim=2),      # Lq no multiple of any tile; the 2-d formula
    "dec_r4": dict(N=2, M=8, D=32, Lq=77, P=4, shapes=PYR, ref_dim=4),      # the 4-d formula; grad_ref[2:]
    "odd": dict(N=1, M=4, D=16, Lq=33, P=2, shapes=[(12, 10), (6, 5)], ref_dim=4),            # L P = 4, M = 4
    "lp6": dict(N=2, M=4, D=8, Lq=21, P=2, shapes=[(12, 10), (6, 5), (3, 4)], ref_dim=2),     # L P not a power of two
    "p1l1": dict(N=1, M=8, D=32, Lq=5, P=1, shapes=[(4, 6)], ref_dim=2),    # softmax of one element: grad_logit exactly 0
    "p8": dict(N=1, M=2, D=8, Lq=19, P=8, shapes=PYR, ref_dim=2),           # L P = 32
    "l16": dict(N=1, M=2, D=4, Lq=9, P=8, shapes=RAGGED16, ref_dim=2),      # L P = 128: more than a wave
    "enc": dict(N=2, M=8, D=32, Lq=S_PYR, P=4, shapes=PYR, ref_dim=2, encoder=True),   # pquad2 forward, sorted2 backward
}
CPU_IDS = [k for k in CASES if k != "enc"]
EXTRA_CASES = {   # beyond the issue's table (emulator only: an odd M L P cannot be a contiguous [N, Lq, 3 M L P], whose ld would be odd)
    # rows M L P odd (5 rows of 3 samples): the epilogue's float2 arrays in LDS start behind an odd count of floats
    "odd_rows": dict(N=1, M=3, D=4, Lq=5, P=1, shapes=[(3, 5)], ref_dim=4),
}


def make(cid, profile):
    """(value, shapes, ref_points, qproj, grad_out) on the CPU and (M, L, P)."""
    kw = CASES[cid] if cid in CASES else EXTRA_CASES[cid]
    value, shapes, refp, qproj = U.make_fused_case(profile, seed=SEED, **kw)
    g = torch.Generator().manual_seed(SEED + 1)
    grad_out = torch.randn(kw["N"], kw["Lq"], kw["M"] * kw["D"], generator=g)
    return (value, shapes, refp, qproj, grad_out), (kw["M"], len(kw["shapes"]), kw["P"])


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else None


def _shape_ptr(shapes):
    flat = [int(v) for hw in (shapes.tolist() if torch.is_tensor(shapes) else shapes) for v in hw]
    return (ctypes.c_int64 * len(flat))(*flat)


def prologue(lib, shapes, refp, qbuf, ld, off_col, logit_col, N, Lq, M, L, P):
    """tf_msda_fused_prologue_f32 on tensors of either library (host tensors: the emulator's) -> (status, loc, attn), both
    NaN-filled before the call."""
    loc = torch.full((N, Lq, M, L, P, 2), float("nan"), dtype=torch.float32, device=refp.device)
    attn = torch.full((N, Lq, M, L, P), float("nan"), dtype=torch.float32, device=refp.device)
    arr = _shape_ptr(shapes)
    rc = lib.tf_msda_fused_prologue_f32(_p(refp), refp.shape[-1], _p(qbuf), ld, off_col, logit_col,
                                        ctypes.cast(arr, ctypes.c_void_p), _p(loc), _p(attn), N, M, L, Lq, P, _stream(refp))
    return rc, loc, attn


def epilogue(lib, shapes, refp, qbuf, ld, off_col, logit_col, attn, gl, ga, gq, ld_g, goff_col, glogit_col, want_ref, M, L, P):
    """tf_msda_fused_backward_epilogue_f32 into the caller's grad_qproj buffer `gq` -> (status, grad_ref or None)."""
    N, Lq = attn.shape[:2]
    gref = torch.full(tuple(refp.shape), float("nan"), dtype=torch.float32, device=refp.device) if want_ref else None
    arr = _shape_ptr(shapes)
    rc = lib.tf_msda_fused_backward_epilogue_f32(_p(refp), refp.shape[-1], _p(qbuf), ld, off_col, logit_col,
                                                 ctypes.cast(arr, ctypes.c_void_p), _p(attn), _p(gl), _p(ga), _p(gq), ld_g, goff_col,
                                                 glogit_col, _p(gref), N, M, L, Lq, P, _stream(refp))
    return rc, gref


# ---- float64 ------------------------------------------------------------------------------------------------------------------------------
def in_range(shapes, loc):
    """The operator kernels' own range test on an fp32 loc [N, Lq, M, L, P, 2] (make_tap: px = fma(loc_x, W, -0.5) rounded ONCE to
    fp32, -1 < px < W, py alike): loc W - 0.5 is exact in float64 (24 + 11 bits), so .float() of it is that one rounding."""
    hw, _ = U._starts(shapes)
    wh = torch.tensor([(w, h) for h, w in hw], dtype=torch.float64, device=loc.device).view(1, 1, 1, len(hw), 1, 2)
    assert loc.dtype == torch.float32
    p = (loc.double() * wh - 0.5).float()
    lim = wh.float()
    return ((p > -1) & (p < lim)).all(-1)


def epilogue_reference(shapes, refp, qproj, attn, gl, ga, M, L, P, loc=None):
    """float64 of the epilogue's formulas on the given (fp32 or float64) inputs -> dict: grad_off (float64 tensor
    [N, Lq, M, L, P, 2]), grad_logit (U.Ref [N, Lq, M, L, P]), grad_ref_xy (U.Ref [N, Lq, L, 2]), grad_ref_wh (U.Ref or None).
    loc: the prologue's fp32 locations -- grad_loc / grad_attn of the samples out of range (in_range) count as zero, whatever
    they hold; None: they are taken as given (float64's own are zero there already)."""
    hw, _ = U._starts(shapes)
    N, Lq = attn.shape[:2]
    LP = L * P
    a, g, l64, r = attn.double(), ga.double(), gl.double(), refp.double()
    if loc is not None:
        inr = in_range(shapes, loc)
        g = torch.where(inr, g, torch.zeros_like(g))
        l64 = torch.where(inr[..., None], l64, torch.zeros_like(l64))
    ah = a.reshape(N, Lq, M, LP)
    gh = g.reshape(N, Lq, M, LP)
    dot = (ah * gh).sum(-1, keepdim=True)
    glogit = (ah * (gh - dot)).reshape(a.shape)
    sc = (ah.abs() * (gh.abs() + (ah.abs() * gh.abs()).sum(-1, keepdim=True))).reshape(a.shape)
    r_logit = U.Ref(glogit, torch.nan_to_num(sc, nan=0.0), torch.full_like(glogit, U.SUB * (LP + 2)), torch.isnan(glogit), LP + 1)
    if r.shape[-1] == 2:
        hws = torch.tensor(hw, dtype=torch.float64, device=a.device)
        goff = l64 / hws.view(1, 1, 1, L, 1, 2)
    else:
        goff = l64 * r[:, :, None, :, None, 2:] * 0.5 / P
    zero = torch.zeros((), dtype=torch.float64, device=a.device)
    sxy = l64.sum((2, 4))
    r_xy = U.Ref(sxy, torch.nan_to_num(l64.abs().sum((2, 4)), nan=0.0), zero, torch.isnan(sxy), M * P)
    r_wh = None
    if r.shape[-1] == 4:
        off = qproj.double()[..., :2 * M * LP].reshape(N, Lq, M, L, P, 2)
        t = l64 * off
        swh = t.sum((2, 4)) * 0.5 / P
        r_wh = U.Ref(swh, torch.nan_to_num(t.abs().sum((2, 4)) * 0.5 / P, nan=0.0), zero, torch.isnan(swh), 2 * M * P)
    return dict(grad_off=goff, grad_logit=r_logit, grad_ref_xy=r_xy, grad_ref_wh=r_wh)


def check_grad_off(y, ref, keep=None, what="grad_off"):
    """|y - ref| <= 2^-22 |ref| + 2^-149 on the kept coordinates, NaN exactly where ref is; returns the worst err / bound."""
    y = y.double().reshape(ref.shape)
    keep = torch.ones_like(ref, dtype=torch.bool) if keep is None else keep
    nan = torch.isnan(ref)
    assert not bool(((torch.isnan(y) != nan) & keep).any()), what + ": NaN outputs differ from the expected ones"
    cmp = keep & ~nan
    assert bool(torch.isfinite(y[cmp]).all()), what + ": non-finite output where none is expected"
    bound = 2.0 ** -22 * ref.abs() + U.SUB
    ratio = torch.where(cmp, (y - ref).abs() / bound, torch.zeros_like(ref))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    assert worst <= 1.0, (what, worst, tuple(int(v) for v in (ratio > 1).nonzero()[0]))
    return worst


def check_epilogue(gq_off, gq_logit, gref, want, keep=None, what=""):
    """grad_off [.., 2], grad_logit and grad_ref of a kernel against epilogue_reference's dict; prints and returns the figures."""
    out = {"grad_off": check_grad_off(gq_off, want["grad_off"], keep, what + " grad_off")}
    out["grad_logit"] = U.check(gq_logit, want["grad_logit"], what=what + " grad_logit").value
    if gref is not None:
        out["grad_ref_xy"] = U.check(gref[..., :2], want["grad_ref_xy"], what=what + " grad_ref[:2]").value
        if want["grad_ref_wh"] is not None:
            out["grad_ref_wh"] = U.check(gref[..., 2:], want["grad_ref_wh"], what=what + " grad_ref[2:]").value
    print(what, " ".join("%s %.3e" % kv for kv in out.items()))
    return out


def check_prologue(loc_k, attn_k, shapes, refp, qproj, M, L, P, what=""):
    """|loc_k - loc| <= dl and |attn_k - a| <= da against U.fused_locations; returns (worst loc err / dl, worst attn err / da)."""
    loc, a, (dlx, dly), da = U.fused_locations(shapes, refp, qproj, M, L, P)
    dl = torch.stack([dlx, dly], -1)
    assert bool(torch.isfinite(loc_k).all()) and bool(torch.isfinite(attn_k).all()), what
    el = (loc_k.double() - loc).abs()
    ea = (attn_k.double() - a).abs()
    assert bool((el <= dl).all()), (what, "loc", float((el - dl).max()))
    assert bool((ea <= da).all()), (what, "attn", float((ea - da).max()))
    wl = float(torch.where(dl > 0, el / dl.clamp_min(1e-300), torch.zeros_like(el)).max())
    wa = float((ea / da).max())
    print(what, "loc err / dl %.3f  attn err / da %.3f" % (wl, wa))
    return wl, wa


def rel_err(y, ref, keep=None):
    """max |y - ref| / max |ref| over the kept elements (the end-to-end figure)."""
    y, ref = y.double().reshape(ref.shape), ref.double()
    d = (y - ref).abs()
    if keep is not None:
        d = torch.where(keep, d, torch.zeros_like(d))
        ref = torch.where(keep, ref, torch.zeros_like(ref))
    m = float(ref.abs().max())
    return float(d.max()) / m if m > 0 else float(d.max())


def bits_equal(a, b):
    """Bit equality (torch.equal would call -0 == +0 and miss a NaN)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
