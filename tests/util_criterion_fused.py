"""The float64 yardstick of the fused set criterion and the matching cost (trackformer_amd/csrc/criterion.h; include/tf_fused.h: THE SET
CRITERION AND THE MATCHING COST), the operand profiles their tests draw from, and the checks both test files share.

THE REFERENCE OF THE FOCAL ELEMENTS IS THE STABLE FORM, not criterion.sigmoid_focal_loss evaluated in float64.  That formulation
builds (1 - p_t)^gamma from 1 - sigmoid(x); even in float64 the subtraction loses the small elements for wide logits (for 8 randn
logits it is 1e-2 relative away from the stable float64 form; for 30 randn the small elements are lost entirely).  With z = x for a
negative and z = -x for a positive element the reference is, in float64,

    focal = a_t softplus(z) exp(-gamma softplus(-z))        softplus(+-z) = max(+-z, 0) + log1p(exp(-|z|))
    d focal / dz = a_t exp(-gamma softplus(-z)) (sigmoid(z) + gamma softplus(z) sigmoid(-z))

A VALUE WITH ITS ERROR SCALE.  Every reference output is written ONCE in terms of `V` = (v, E): v the float64 value, E the scale an fp32
evaluation's error is measured in.  Leaves (the fp32 operands) have E = 0 and every operation adds its own result:

    E(a o b) = |d/da| E(a) + |d/db| E(b) + |result|

Multiplication by 0.5, by a sign and negation are exact.  max / min / clamp / where take the E of the operand that is taken (for max:
the larger one): a clamp that lands on its bound is exact.  The scale S of an output is then the E of its own expression -- the
analytic box gradients included, which tests/test_criterion_fused_cpu.py checks against float64 autograd through
box_ops.generalized_box_iou_pairs.  Two scales are stated directly instead:

    focal elements and their gradients    S = |ref| (1 + gamma |log(1 - p_t)|)     the argument rounding of the exp is the only amplification
    a cost entry                          S = |w_bbox| S_l1 + |w_class| S_class + |w_giou| S_giou

The sums of the losses are accumulated in fp64 by the kernel and rounded once: a sum's E is the sum of its elements' E plus its own
result, and no sqrt(n) growth enters.

    (|got - ref| - 4 . 2^-149) / S  <=  util_split_numerics.BOUND = 2^-20        no element exempt

SECOND CRITERION, as everywhere in this project: the worst normalised excess is at most FP32_FACTOR (4) x that of torch's own fp32
formulation (SetCriterion._layers_at_once, HungarianMatcher._cost_torch; on the CPU) on the same operands, or FP32_CLASS_MIN.  It is
applied ONLY WHERE TORCH'S OWN EXCESS IS ITSELF <= BOUND: on logits of 8 randn and wider torch's focal formulation exceeds the bound
by four orders of magnitude and bounds nothing (measured with this recipe, torch fp32 on the CPU: randn logits 1.87 x 2^-20, 8 randn
7e4 to 1.2e5 x 2^-20; the stable form in fp32 <= 0.18 (losses) and <= 0.26 (gradients) on every profile).  For the box terms it is the
binding one (torch fp32 GIoU loss 0.008 to 0.016 x 2^-20, gradient 0.004 to 0.011).

TIES.  The gradients of L1 and GIoU are discontinuous where two coordinates or corners coincide or an intersection is exactly empty.
matched_boxes() and Case redraw every matched pair with a coordinate difference, a corner difference or an intersection extent below MARGIN = 2^-10
(times the profile's size factor: 1e-3 for the 1e-3-sized boxes, whose extents are themselves below 2^-10), and every row whose two
largest logits are closer than MARGIN (times the profile's scale), until none is left; nothing is skipped or filtered afterwards, and
margins() is asserted by the tests.

THE KERNELS' OWN FIGURES, first run on an MI355X (tests/test_criterion_fused_gpu.py, tests/test_matcher_fused_cost_gpu.py; worst
normalised excess over all their cases in units of 2^-20): losses 0.027 (unit logits; 0.019 wide, 0.008 tiny), logit gradients 0.305
(wide; 0.237 unit, 0.158 tiny), box gradients 0.012, cardinality 0.041, class error 0.040, cost entries 0.029 (wide; 0.018 unit, 0.020
tiny); the emulated library (the host's libm) stays below the same figures within 0.05.

Everything here is torch, float64, and runs on the CPU or the device."""
import math

import numpy as np
import torch

from tests import util_split_numerics as U
from trackformer_amd import box_ops
from trackformer_amd.criterion import SetCriterion
from trackformer_amd.matcher import HungarianMatcher

BOUND, FP32_FACTOR, FP32_CLASS_MIN = U.BOUND, U.FP32_FACTOR, U.FP32_CLASS_MIN
FLOOR = 4 * 2.0 ** -149
MARGIN = 2.0 ** -10
LOGIT_PROFILES = {"unit": 1.0, "wide": 30.0, "tiny": 1e-4}
BOX_PROFILES = {"overlapping": 1.0, "disjoint": 1.0, "nested": 1.0, "small": 1e-3}
OUTPUTS = ("losses", "card", "class_error", "grad_logits", "grad_boxes")


# ---- the value-with-error-scale type -------------------------------------------------------------------------------------------------
class V:
    """(v, E): a float64 value and the scale of an fp32 evaluation's error (module docstring)."""
    __slots__ = ("v", "E")

    def __init__(self, v, E=None):
        self.v = v if torch.is_tensor(v) else torch.tensor(float(v), dtype=torch.float64)
        self.v = self.v.double()
        self.E = torch.zeros_like(self.v) if E is None else E.double()

    @staticmethod
    def of(x, like=None):
        if isinstance(x, V):
            return x
        t = torch.as_tensor(x, dtype=torch.float64)
        return V(t.to(like.v.device) if like is not None else t)

    def __add__(self, o):
        o = V.of(o, self)
        r = self.v + o.v
        return V(r, self.E + o.E + r.abs())

    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o, self)
        r = self.v - o.v
        return V(r, self.E + o.E + r.abs())

    def __rsub__(self, o):
        return V.of(o, self) - self

    def __mul__(self, o):
        o = V.of(o, self)
        r = self.v * o.v
        return V(r, o.v.abs() * self.E + self.v.abs() * o.E + r.abs())

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o, self)
        r = self.v / o.v
        return V(r, self.E / o.v.abs() + (self.v / (o.v * o.v)).abs() * o.E + r.abs())

    def __rtruediv__(self, o):
        return V.of(o, self) / self

    def __neg__(self):
        return V(-self.v, self.E)

    def exact(self, factor):
        """Times an exactly representable factor whose product is exact: 0.5, a sign, 0, 1."""
        f = torch.as_tensor(factor, dtype=torch.float64, device=self.v.device)
        return V(self.v * f, self.E * f.abs())

    def abs(self):
        return V(self.v.abs(), self.E)

    def exp(self):
        r = self.v.exp()
        return V(r, r * self.E + r)

    def log(self):
        r = self.v.log()
        return V(r, self.E / self.v.abs() + r.abs())

    def log1p(self):
        r = self.v.log1p()
        return V(r, self.E / (1 + self.v).abs() + r.abs())

    def pow(self, g):
        r = self.v.pow(g)
        return V(r, (g * self.v.pow(g - 1)).abs() * self.E + r.abs())

    @staticmethod
    def where(cond, a, b):
        a, b = V.of(a), V.of(b)
        return V(torch.where(cond, a.v, b.v), torch.where(cond, a.E, b.E))

    def maximum(self, o):
        o = V.of(o, self)
        return V.where(self.v >= o.v, self, o)

    def minimum(self, o):
        o = V.of(o, self)
        return V.where(self.v <= o.v, self, o)

    def clamp_min0(self):
        return V.where(self.v >= 0, self, V(torch.zeros_like(self.v)))

    def sum(self, dims):
        """A sum accumulated wider than fp32 and rounded once: the elements' E plus the result."""
        r = self.v.sum(dims)
        return V(r, self.E.sum(dims) + r.abs())

    def __getitem__(self, idx):
        return V(self.v[idx], self.E[idx])


def stack(vs, dim=-1):
    return V(torch.stack([x.v for x in vs], dim), torch.stack([x.E for x in vs], dim))


# ---- operands --------------------------------------------------------------------------------------------------------------------------
def _top2_gap(x):
    if x.shape[-1] < 2:
        return torch.full(x.shape[:-1], math.inf)
    t = x.double().topk(2, -1).values
    return t[..., 0] - t[..., 1]


def logits(profile, shape, gen):
    """Seeded logits [..., C] for `profile`; rows whose two largest values are closer than MARGIN x scale are redrawn."""
    scale = LOGIT_PROFILES[profile]
    x = torch.randn(shape, generator=gen) * scale
    while True:
        bad = _top2_gap(x) < MARGIN * scale
        if not bool(bad.any()):
            return x
        x[bad] = torch.randn((int(bad.sum()), shape[-1]), generator=gen) * scale


def _rand(gen, n, lo, hi):
    return torch.rand(n, generator=gen) * (hi - lo) + lo


def _draw_partner(profile, tb, gen):
    """A prediction box [n, 4] (cxcywh, at unit size) for every target box tb [n, 4] of `profile`."""
    n = tb.shape[0]
    cx, cy, w, h = tb.unbind(-1)
    if profile in ("overlapping", "small"):
        return torch.stack([cx + _rand(gen, n, -0.3, 0.3) * w, cy + _rand(gen, n, -0.3, 0.3) * h,
                            w * _rand(gen, n, 0.7, 1.4), h * _rand(gen, n, 0.7, 1.4)], -1)
    if profile == "disjoint":
        w2, h2 = w * _rand(gen, n, 0.7, 1.4), h * _rand(gen, n, 0.7, 1.4)
        side = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
        return torch.stack([cx + side * (0.5 * (w + w2) + _rand(gen, n, 0.05, 0.2)), cy + _rand(gen, n, -0.5, 0.5) * h, w2, h2], -1)
    if profile == "nested":
        inner = torch.stack([cx + _rand(gen, n, -0.12, 0.12) * w, cy + _rand(gen, n, -0.12, 0.12) * h,
                             w * _rand(gen, n, 0.3, 0.7), h * _rand(gen, n, 0.3, 0.7)], -1)
        outer = torch.stack([cx + _rand(gen, n, -0.12, 0.12) * w, cy + _rand(gen, n, -0.12, 0.12) * h,
                             w * _rand(gen, n, 1.4, 2.0), h * _rand(gen, n, 1.4, 2.0)], -1)
        return torch.where((torch.rand(n, generator=gen) < 0.5)[:, None], inner, outer)
    raise ValueError(profile)


def _shrink(b, size):
    """Unit-size geometry -> the profile's size: the same picture scaled about (0.5, 0.5)."""
    if size == 1.0:
        return b
    return torch.cat([0.5 + (b[:, :2] - 0.5) * size, b[:, 2:] * size], -1)


def _xyxy(b):
    return torch.stack([b[..., 0] - 0.5 * b[..., 2], b[..., 1] - 0.5 * b[..., 3], b[..., 0] + 0.5 * b[..., 2], b[..., 1] + 0.5 * b[..., 3]], -1)


def pair_margins(a, b):
    """The smallest distance [n] of the matched pairs a, b [n, 4] (fp32 cxcywh) from a tie of the L1 or GIoU gradient: coordinate
    differences, corner differences and the raw extents of the intersection, in float64 arithmetic on the fp32 values."""
    a, b = a.double(), b.double()
    xa, xb = _xyxy(a), _xyxy(b)
    iw = torch.minimum(xa[:, 2], xb[:, 2]) - torch.maximum(xa[:, 0], xb[:, 0])
    ih = torch.minimum(xa[:, 3], xb[:, 3]) - torch.maximum(xa[:, 1], xb[:, 1])
    return torch.cat([(a - b).abs(), (xa - xb).abs(), iw.abs()[:, None], ih.abs()[:, None]], -1).min(-1).values


def matched_boxes(profile, n, gen):
    """(prediction boxes [n, 4], target boxes [n, 4]) of `profile`, fp32 cxcywh; pairs closer than MARGIN x size to a tie are redrawn."""
    size = BOX_PROFILES[profile]
    tb = torch.stack([_rand(gen, n, 0.3, 0.7), _rand(gen, n, 0.3, 0.7), _rand(gen, n, 0.1, 0.3), _rand(gen, n, 0.1, 0.3)], -1)
    a = _draw_partner(profile, tb, gen)
    sa, sb = _shrink(a, size), _shrink(tb, size)
    while n:
        bad = pair_margins(sa, sb) < MARGIN * size
        if not bool(bad.any()):
            break
        a[bad] = _draw_partner(profile, tb[bad], gen)
        sa = _shrink(a, size)
    return sa, sb


class Case:
    """One seeded problem: logits [L, B, Q, C], boxes [L, B, Q, 4], the targets and a random matching of every layer (the same number
    of pairs per image in every layer)."""

    def __init__(self, L, B, Q, C, per_image, logit_profile="unit", box_profile="overlapping", seed=0, device="cpu"):
        gen = torch.Generator().manual_seed(1000003 * seed + 7919 * L + 101 * B + 13 * Q + C)
        per_image = list(per_image)
        assert len(per_image) == B
        self.L, self.B, self.Q, self.C, self.sizes = L, B, Q, C, per_image
        self.logit_profile, self.box_profile = logit_profile, box_profile
        self.T = T = sum(per_image)
        size = BOX_PROFILES[box_profile]
        self.logits = logits(logit_profile, (L, B, Q, C), gen)
        free = torch.stack([_rand(gen, L * B * Q, 0.2, 0.8), _rand(gen, L * B * Q, 0.2, 0.8), _rand(gen, L * B * Q, 0.05, 0.4),
                            _rand(gen, L * B * Q, 0.05, 0.4)], -1)
        self.boxes = _shrink(free, size).reshape(L, B, Q, 4).contiguous()
        self.labels = torch.randint(0, C, (T,), generator=gen, dtype=torch.int64)
        self.tboxes = torch.zeros(T, 4)
        self.tgt_of = torch.full((L, B, Q), -1, dtype=torch.int32)
        self.all_indices = []
        offs = np.concatenate([[0], np.cumsum(per_image)[:-1]]).astype(np.int64)
        pairs = []   # (l, b, q, t)
        for l in range(L):
            ind = []
            for b, n in enumerate(per_image):
                m = min(n, Q)
                src = torch.randperm(Q, generator=gen)[:m].sort().values
                tgt = torch.randperm(n, generator=gen)[:m]
                ind.append((src, tgt))
                pairs += [(l, b, int(q), int(t) + int(offs[b])) for q, t in zip(src, tgt)]
            self.all_indices.append(ind)
        # every target box is drawn once; each prediction matched to it is drawn as its partner
        if T:
            self.tboxes = matched_boxes(box_profile, T, gen)[1]
        if pairs:
            idx = torch.tensor(pairs)
            tb_unit = torch.cat([0.5 + (self.tboxes[:, :2] - 0.5) / size, self.tboxes[:, 2:] / size], -1)[idx[:, 3]]
            a = _draw_partner(box_profile, tb_unit, gen)
            while True:
                bad = pair_margins(_shrink(a, size), self.tboxes[idx[:, 3]]) < MARGIN * size
                if not bool(bad.any()):
                    break
                a[bad] = _draw_partner(box_profile, tb_unit[bad], gen)
            self.boxes[idx[:, 0], idx[:, 1], idx[:, 2]] = _shrink(a, size)
            self.tgt_of[idx[:, 0], idx[:, 1], idx[:, 2]] = idx[:, 3].to(torch.int32)
        self.tgt_len = torch.tensor(per_image, dtype=torch.int32)
        self.num_boxes = float(max(T, 1))
        self.G = torch.rand(L, 3, generator=gen) + 0.5          # the weights of a random weighted sum of the losses
        if device != "cpu":
            for k in ("logits", "boxes", "labels", "tboxes", "tgt_of", "tgt_len", "G"):
                setattr(self, k, getattr(self, k).to(device))

    def margins(self):
        """(smallest tie distance of the matched pairs / (MARGIN x size), smallest top-2 logit gap / (MARGIN x scale)): both >= 1."""
        m = self.tgt_of >= 0
        box = math.inf
        if bool(m.any()):
            box = float(pair_margins(self.boxes[m].cpu(), self.tboxes.cpu()[self.tgt_of[m].long().cpu()]).min())
        return (box / (MARGIN * BOX_PROFILES[self.box_profile]),
                float(_top2_gap(self.logits.cpu()).min()) / (MARGIN * LOGIT_PROFILES[self.logit_profile]))

    def targets(self, device=None):
        """The targets as the criterion takes them: a list of {"labels", "boxes"} per image."""
        out, o = [], 0
        for n in self.sizes:
            out.append({"labels": self.labels[o:o + n].to(device or self.labels.device),
                        "boxes": self.tboxes[o:o + n].to(device or self.tboxes.device)})
            o += n
        return out

    def layer_outputs(self, lg=None, bx=None):
        lg = self.logits if lg is None else lg
        bx = self.boxes if bx is None else bx
        return [{"pred_logits": lg[l], "pred_boxes": bx[l]} for l in range(self.L)]


def criterion_for(C, alpha, gamma):
    """A focal SetCriterion over C classes with the three losses the fused route covers."""
    matcher = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0, focal_loss=True, focal_alpha=alpha if alpha >= 0 else 0.25,
                               focal_gamma=gamma)
    return SetCriterion(C, matcher, {}, 0.1, ["labels", "boxes", "cardinality"], True, alpha, gamma, False, 0.0)


# ---- the references ----------------------------------------------------------------------------------------------------------------------
def _softplus_parts(z):
    u = (-z.abs()).exp().log1p()
    return z.clamp_min(0) + u, (-z).clamp_min(0) + u          # softplus(z), softplus(-z)


def focal_reference(x, pos, alpha, gamma):
    """(loss V, d loss / dx V) of the focal elements in the stable float64 form; x float64 [...], pos bool [...]."""
    z = torch.where(pos, -x, x)
    sp, sn = _softplus_parts(z)
    mod = (-gamma * sn).exp()
    a = torch.ones_like(x) if alpha < 0 else torch.where(pos, torch.full_like(x, alpha), torch.full_like(x, 1 - alpha))
    loss = a * sp * mod
    dz = a * mod * (torch.sigmoid(z) + gamma * sp * torch.sigmoid(-z))
    amp = 1 + gamma * sn
    dx = torch.where(pos, -dz, dz)
    return V(loss, loss.abs() * amp), V(dx, dx.abs() * amp)


def _corners(b):
    """cxcywh V [..., 4] -> (x1, y1, x2, y2) as V."""
    cx, cy, w, h = (b[..., k] for k in range(4))
    return cx - w.exact(0.5), cy - h.exact(0.5), cx + w.exact(0.5), cy + h.exact(0.5)


def giou_reference(a, b, grad=False):
    """GIoU of the cxcywh pairs a, b (V [n, 4]) operation by operation as box_ops.generalized_box_iou_pairs -> V [n]; grad: also the
    analytic gradient of (1 - GIoU) with respect to a, V [n, 4]."""
    ax1, ay1, ax2, ay2 = _corners(a)
    bx1, by1, bx2, by2 = _corners(b)
    w1, h1 = ax2 - ax1, ay2 - ay1
    area1, area2 = w1 * h1, (bx2 - bx1) * (by2 - by1)
    iwr, ihr = ax2.minimum(bx2) - ax1.maximum(bx1), ay2.minimum(by2) - ay1.maximum(by1)
    iw, ih = iwr.clamp_min0(), ihr.clamp_min0()
    inter = iw * ih
    uni = area1 + area2 - inter
    hwr, hhr = ax2.maximum(bx2) - ax1.minimum(bx1), ay2.maximum(by2) - ay1.minimum(by1)
    hw, hh = hwr.clamp_min0(), hhr.clamp_min0()
    hull = hw * hh
    giou = inter / uni - (hull - uni) / hull
    if not grad:
        return giou
    g_uni = 1.0 / hull - inter / (uni * uni)
    g_inter = 1.0 / uni - g_uni
    g_hull = -(uni / (hull * hull))
    zero = V(torch.zeros_like(giou.v))
    g_iw, g_ih = V.where(iwr.v >= 0, g_inter * ih, zero), V.where(ihr.v >= 0, g_inter * iw, zero)
    g_hw, g_hh = V.where(hwr.v >= 0, g_hull * hh, zero), V.where(hhr.v >= 0, g_hull * hw, zero)

    def lt(p, q):   # the share of min(p, q) / max(q, p) that goes to p
        return torch.where(p.v < q.v, 1.0, torch.where(p.v == q.v, 0.5, 0.0))
    gx2 = (g_iw.exact(lt(ax2, bx2)) + g_hw.exact(lt(bx2, ax2))) + g_uni * h1
    gx1 = -((g_iw.exact(lt(bx1, ax1)) + g_hw.exact(lt(ax1, bx1))) + g_uni * h1)
    gy2 = (g_ih.exact(lt(ay2, by2)) + g_hh.exact(lt(by2, ay2))) + g_uni * w1
    gy1 = -((g_ih.exact(lt(by1, ay1)) + g_hh.exact(lt(ay1, by1))) + g_uni * w1)
    return giou, stack([-(gx1 + gx2), -(gy1 + gy2), -((gx2 - gx1).exact(0.5)), -((gy2 - gy1).exact(0.5))])


def _argmax_lowest(x):
    """arg-max over the last dimension, the lowest index on ties."""
    C = x.shape[-1]
    top = x.max(-1, keepdim=True).values
    idx = torch.arange(C, device=x.device).expand_as(x)
    return torch.where(x == top, idx, torch.full_like(idx, C)).min(-1).values


def reference(case, alpha, gamma, tgt_of=None):
    """{name: V} for the five outputs of the two criterion entries, float64 on the case's device; the gradients are those of
    sum(G * losses).  tgt_of: another matching than the case's own (the self-tests)."""
    L, B, Q, C = case.L, case.B, case.Q, case.C
    tgt_of = (case.tgt_of if tgt_of is None else tgt_of).long()
    x = case.logits.double()
    m = tgt_of >= 0
    nb = V(torch.tensor(case.num_boxes, dtype=torch.float64, device=x.device))
    label = torch.full((L, B, Q), -1, dtype=torch.int64, device=x.device)
    if case.T:
        label[m] = case.labels[tgt_of[m]]
    pos = torch.arange(C, device=x.device).expand(L, B, Q, C) == label[..., None]
    f, df = focal_reference(x, pos, alpha, gamma)
    loss_ce = f.sum((1, 2, 3)) / nb
    G = V(case.G.double())
    g = G / nb                                                     # [L, 3]
    gl = df.v * g.v[:, 0, None, None, None]
    sp, sn = _softplus_parts(torch.where(pos, -x, x))
    grad_logits = V(gl, gl.abs() * (1 + gamma * sn))
    # the matched pairs
    lay = torch.arange(L, device=x.device)[:, None, None].expand(L, B, Q)[m]
    a = V(case.boxes.double()[m])
    b = V(case.tboxes.double()[tgt_of[m]]) if case.T else V(torch.zeros(0, 4, dtype=torch.float64, device=x.device))
    d = a - b
    l1 = ((d[:, 0].abs() + d[:, 1].abs()) + d[:, 2].abs()) + d[:, 3].abs()
    giou, ggrad = giou_reference(a, b, grad=True)
    lg = 1.0 - giou
    onehot = (lay[:, None] == torch.arange(L, device=x.device)[None]).double()          # [n, L]
    loss_bbox = V(onehot.t() @ l1.v, onehot.t() @ l1.E)
    loss_bbox = V(loss_bbox.v, loss_bbox.E + loss_bbox.v.abs()) / nb
    loss_giou = V(onehot.t() @ lg.v, onehot.t() @ lg.E)
    loss_giou = V(loss_giou.v, loss_giou.E + loss_giou.v.abs()) / nb
    gb_rows = (g[:, 1][lay][:, None]).exact(torch.sign(d.v)) + ggrad * g[:, 2][lay][:, None] if int(m.sum()) else None
    gb = V(torch.zeros(L, B, Q, 4, dtype=torch.float64, device=x.device))
    if gb_rows is not None:
        gb.v[m], gb.E[m] = gb_rows.v, gb_rows.E
    # cardinality and class error: counts
    arg = _argmax_lowest(x)
    cnt = (arg != C - 1).sum(2).double()                           # [L, B]
    card = V((cnt - case.tgt_len.double()[None]).abs().sum(1)) / V(torch.tensor(float(B), dtype=torch.float64, device=x.device))
    n = int(m[0].sum())
    if n:
        ok = float((arg[0][m[0]] == label[0][m[0]]).sum())
        ce = 100.0 - V(torch.tensor([ok], device=x.device)) * (V(torch.tensor([100.0], device=x.device)) / float(n))
    else:
        ce = V(torch.tensor([100.0], dtype=torch.float64, device=x.device))
    return {"losses": stack([loss_ce, loss_bbox, loss_giou]), "card": card, "class_error": ce, "grad_logits": grad_logits, "grad_boxes": gb}


def fp32_formulation(case, alpha, gamma):
    """torch's own fp32 formulation of the same outputs, on the CPU: SetCriterion._layers_at_once and autograd through it."""
    crit = criterion_for(case.C, alpha, gamma)
    with torch.enable_grad():
        lg = case.logits.detach().cpu().clone().requires_grad_(True)
        bx = case.boxes.detach().cpu().clone().requires_grad_(True)
        out = crit._layers_at_once(case.layer_outputs(lg, bx), case.targets("cpu"), case.all_indices, case.num_boxes)
        losses, card = dict_to_tensors(out, case.L)
        gl, gb = torch.autograd.grad((losses * case.G.cpu()).sum(), (lg, bx), allow_unused=True)
    gb = torch.zeros_like(bx) if gb is None else gb
    return {"losses": losses.detach(), "card": card, "class_error": out["class_error"].reshape(1), "grad_logits": gl, "grad_boxes": gb}


def dict_to_tensors(out, L):
    """The criterion's dict -> (losses [L, 3], card [L]) in the entry's layout."""
    suffix = [""] + ["_%d" % i for i in range(L - 1)]
    losses = torch.stack([torch.stack([out["loss_ce" + s], out["loss_bbox" + s], out["loss_giou" + s]]) for s in suffix])
    return losses, torch.stack([out["cardinality_error" + s] for s in suffix])


def cost_reference(lg, boxes, tgt_ids, tgt_bbox, w_class, w_bbox, w_giou, alpha, gamma):
    """The focal matching cost [R, T] as V, float64: the matcher's formula with its +1e-8 inside both logarithms."""
    R, T = lg.shape[0], tgt_ids.numel()
    x = V(lg.double()[:, tgt_ids])
    e = (-x.abs()).exp()
    inv = 1.0 / (1.0 + e)
    p = V.where(x.v >= 0, inv, e * inv)
    q = V.where(x.v >= 0, e * inv, inv)
    neg = ((1.0 - V.of(alpha)) * p.pow(gamma)) * -((q + 1e-8).log())
    pos = (V.of(alpha) * q.pow(gamma)) * -((p + 1e-8).log())
    c_class = pos - neg
    a = V(boxes.double()[:, None, :].expand(R, T, 4).reshape(-1, 4))
    b = V(tgt_bbox.double()[None, :, :].expand(R, T, 4).reshape(-1, 4))
    d = a - b
    l1 = ((d[:, 0].abs() + d[:, 1].abs()) + d[:, 2].abs()) + d[:, 3].abs()
    giou = giou_reference(a, b)
    v = w_bbox * l1.v.view(R, T) + w_class * c_class.v + w_giou * -giou.v.view(R, T)
    return V(v, abs(w_bbox) * l1.E.view(R, T) + abs(w_class) * c_class.E + abs(w_giou) * giou.E.view(R, T))


def cost_fp32(lg, boxes, tgt_ids, tgt_bbox, w_class, w_bbox, w_giou, alpha, gamma):
    """torch's own fp32 chain of the same cost on the CPU (HungarianMatcher._cost_torch)."""
    mt = HungarianMatcher(w_class, w_bbox, w_giou, True, alpha, gamma)
    with torch.no_grad():
        return mt._cost_torch(lg.cpu().float(), boxes.cpu().float(), tgt_ids.cpu(), tgt_bbox.cpu().float())


# ---- the checks --------------------------------------------------------------------------------------------------------------------------
def excess_of(got, ref, fp32=None):
    _, worst = U.excess(got, ref.v, ref.E, torch.full_like(ref.v, FLOOR), None, fp32)
    return worst


def check_one(name, got, ref, fp32, what=""):
    """Both criteria for one output (module docstring); prints the figures (pytest -s) before it asserts."""
    if ref.v.numel() == 0:
        assert got.numel() == 0
        return None
    worst = excess_of(got, ref, fp32)
    second = fp32 is not None and worst.fp32_err <= BOUND
    print("%-58s %-12s %.3f x 2^-20 (torch fp32: %.3g x 2^-20%s)" % (what, name, worst.value / BOUND, worst.fp32_err / BOUND,
                                                                     "" if second else ", bounds nothing"))
    assert worst.value <= BOUND, (what, name, worst)
    if second:
        assert worst.value <= max(FP32_FACTOR * worst.fp32_err, FP32_CLASS_MIN), (what, name, worst)
    return worst


def check(got, ref, fp32, what=""):
    """check_one for every output in `got` ({name: tensor}) -> {name: Excess}."""
    return {name: check_one(name, got[name].cpu(), V(ref[name].v.cpu(), ref[name].E.cpu()), None if fp32 is None else fp32[name], what)
            for name in OUTPUTS if got.get(name) is not None}


def perturbed_assignments(cost, sizes, B, Q, seed, copies=8):
    """linear_sum_assignment of the float64 cost V [B * Q, T] per image, and of `copies` copies perturbed by +- its own bound (BOUND . S +
    FLOOR, a random sign per element) -> (pairs of the unperturbed cost, True when every copy gives the same pairs)."""
    from scipy.optimize import linear_sum_assignment
    gen = torch.Generator().manual_seed(seed)
    c = cost.v.cpu().view(B, Q, -1)
    e = (BOUND * cost.E.cpu() + FLOOR).view(B, Q, -1)

    def solve(m):
        return [tuple(np.asarray(i).tolist() for i in linear_sum_assignment(blk[b].numpy())) for b, blk in enumerate(m.split(sizes, -1))]
    base = solve(c)
    same = True
    for _ in range(copies):
        sign = torch.where(torch.rand(c.shape, generator=gen) < 0.5, -1.0, 1.0).double()
        same = same and solve(c + sign * e) == base
    return base, same
